/*
 * bhrt_api.c -- host side of libbhrt.so, in C (C11), calling HIP through the C runtime API
 * and the two launchers of geodesic.hip.
 *
 * Drop-in entry points keep the reference's argument checks and return codes
 * (src/raytracer.c, src/blackhole_api.c); the ray tracing itself always runs on the GPU.
 * There is no CPU fallback: a HIP failure is reported through the reference's error value
 * (RAY_ERROR / -1 / BH_ERROR_SIMULATION) and bhrt_last_error().
 *
 * Device state is per (host thread, device): a stream, growable device buffers and a ring
 * of control blocks (queue head + counters) with start/stop events per launch, so
 * trace_ray / trace_rays_batch stay callable concurrently from several host threads
 * (SURVEY.md 8b "Threading").
 */
#define _GNU_SOURCE
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#pragma GCC visibility push(default)
#include "../../include/bhrt_api.h"
#pragma GCC visibility pop
#include "bhrt_host.h"
#include "bhrt_kernel.h"

/* ======================================================================================= */
/* errors                                                                                  */
/* ======================================================================================= */
static _Thread_local char g_err[256];

void bhrt_set_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    if (getenv("BHRT_VERBOSE")) fprintf(stderr, "libbhrt: %s\n", g_err);
}
#define set_err bhrt_set_err

const char* bhrt_last_error(void) { return g_err; }

#define HIP_TRY(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_err("%s failed: %s", #call, hipGetErrorString(e_));                           \
            return -1;                                                                        \
        }                                                                                     \
    } while (0)

/* ======================================================================================= */
/* host vector helpers (math_util.c:31-122 semantics; also the drop-in vector3D_* symbols)  */
/* ======================================================================================= */
Vector3D vector3D_add(const Vector3D a, const Vector3D b) {
    Vector3D r = {a.x + b.x, a.y + b.y, a.z + b.z};
    return r;
}
Vector3D vector3D_sub(const Vector3D a, const Vector3D b) {
    Vector3D r = {a.x - b.x, a.y - b.y, a.z - b.z};
    return r;
}
Vector3D vector3D_scale(const Vector3D v, double s) {
    Vector3D r = {v.x * s, v.y * s, v.z * s};
    return r;
}
double vector3D_dot(const Vector3D a, const Vector3D b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
Vector3D vector3D_cross(const Vector3D a, const Vector3D b) {
    Vector3D r = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
    return r;
}
double vector3D_length(const Vector3D v) { return sqrt(vector3D_dot(v, v)); }
Vector3D vector3D_normalize(const Vector3D v) {
    double l = vector3D_length(v);
    if (l < BH_EPSILON) {
        Vector3D z = {0.0, 0.0, 0.0};
        return z;
    }
    return vector3D_scale(v, 1.0 / l);
}
double clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* ======================================================================================= */
/* device contexts                                                                          */
/* ======================================================================================= */
#define BHRT_MAX_DEV 16
/* control blocks per context: a launch into a full ring first harvests its older half (the
 * launches BHRT_RING / 2 and more back, long finished when frames are in flight: the newer half
 * keeps the GPU busy meanwhile; harvesting every launch drained the GPU once per BHRT_RING
 * launches, C4 8-GPU shard -1.2%, profiles/r06/ab_half_harvest.txt). 256 slots of 16.6 KB:
 * 4.26 MB per context, i.e. per host thread and device */
#ifndef BHRT_RING
#define BHRT_RING 256
#endif
#define BHRT_CTL_WORDS 16   /* u64 per control block (128 B): [1..5] counters, [6..7] redo,
                               [8..10] the launch's execution window (geodesic.hip k_trace) */
#define BHRT_QWORDS ((1 << BHRT_MAX_QUEUE_BITS) * BHRT_QUEUE_STRIDE_MAX) /* queue heads per block */
/* a launch's control block and its ray-queue heads are one region of the ring: 64 B of
 * counters, padding to 256 B, then the queue heads. The whole ring is zeroed by one fill on the
 * GPU after each harvest (ring_order), never per launch. */
#define BHRT_QHEAD_OFF 32 /* u64 words */
#define BHRT_SLOT_WORDS (BHRT_QHEAD_OFF + BHRT_QWORDS)
#define BHRT_RING_BYTES ((size_t)BHRT_RING * BHRT_SLOT_WORDS * sizeof(unsigned long long))
#define BHRT_RING_STREAMS 8 /* streams remembered as ordered after the ring's last fill */
#define BHRT_MAX_CHUNKS 8   /* host-buffer frames: pipelined chunks per device            */
#define BHRT_SCRATCH_SLOTS 8
#define BHRT_FRAME_SLOTS 3  /* host-buffer frames in flight per thread (bhrt_render_frame_async) */
#define BHRT_COPY_PARTS 4   /* host-buffer frames: a chunk's D2H in parts, each un-permuted as it lands */
#define BHRT_NFIELDS 15

typedef struct {
    int slot;
    int redo; /* the redo pass was launched after the hot one */
    int untested; /* RKF45 attempts without the accept test (bhrt_scene_k.accept_all) */
    hipEvent_t ev0, ev1;
} pending_t;

typedef struct {
    int device;
    hipStream_t stream;
    unsigned long long* d_ctl; /* BHRT_RING x BHRT_SLOT_WORDS: control block + queue heads */
    pending_t pend[BHRT_RING];
    int npend, next_slot;
    hipEvent_t evpool[2 * BHRT_RING];
    double clock_khz; /* the device's wall-clock rate (hipDeviceAttributeWallClockRate), 0: unknown */
    /* the ring's zeroing (ring_order): ring_dirty = harvested, not yet zeroed; ring_ev = the
     * fill's completion on the stream it ran on; ring_ok = streams already ordered after it */
    int ring_dirty, n_ring_ok;
    int dirty_row, dirty_rows; /* the slots the next fill zeroes (harvest) */
    hipEvent_t ring_ev;
    hipStream_t ring_ok[BHRT_RING_STREAMS];
    /* pinned staging for the ring's counter words (harvest) */
    unsigned long long* h_ctl;
    /* NULL hip_stream of the device API (null_fence): the caller's default stream -> libbhrt's
     * stream before the launch, and back after it */
    hipEvent_t nul_in, nul_out;
    /* growable device buffers */
    void* d_rays;
    size_t cap_rays;
    void* d_soa;
    size_t cap_soa; /* rays */
    void* h_stage;  /* pinned staging for SoA readback */
    size_t cap_stage;
    void* h_rays;   /* pinned staging for ray uploads (trace_rays_batch) */
    size_t cap_hrays;
    /* per-stream launch scratch (ray-array init table + redo list), so launches on different
     * streams never share it; a slot moves to another stream only after its stream drained */
    struct {
        hipStream_t stream;
        void* p;
        size_t cap;
    } scratch[BHRT_SCRATCH_SLOTS];
    int scratch_next;
    /* host-buffer frames (bhrt_render_frame): two trace streams for overlapping chunks, a
     * copy stream, and per chunk: trace finished / its D2H landed */
    hipStream_t stream2, copy;
    hipStream_t xs[2]; /* trace streams 3 and 4 of pipelined ray batches (created on first use) */
    hipEvent_t tev[BHRT_MAX_CHUNKS][4]; /* BHRT_HOST_TIMING=2: per batch chunk, timing events
                                           (upload issued, uploaded, traced, downloaded) */
    hipEvent_t tev0;
    hipEvent_t chunk_done[BHRT_MAX_CHUNKS], chunk_copied[BHRT_MAX_CHUNKS];
    /* per frame slot of bhrt_render_frame_async: device SoA of every chunk, pinned staging
     * of the caller's fields, chunk traced / chunk copied */
    struct {
        void* d_soa;
        size_t cap_soa;
        void* h_stage;
        size_t cap_stage;
        hipEvent_t done[BHRT_MAX_CHUNKS], copied[BHRT_MAX_CHUNKS];
        hipEvent_t part[BHRT_MAX_CHUNKS][BHRT_COPY_PARTS]; /* part p of chunk k landed */
    } fr[BHRT_FRAME_SLOTS];
    /* busy span of the trace kernels since the last stats reset: span_ref is recorded before
     * the first launch; [span_lo, span_hi] = earliest start / latest end relative to it (ms).
     * With launches overlapping on several streams, span / launches is the GPU time per
     * launch that the per-launch HIP-event durations (which overlap) cannot give. */
    hipEvent_t span_ref;
    int span_on;
    double span_lo, span_hi;
    /* bhrt_render_frame_gather: this device's shard buffers; g_done = its shards rendered;
     * g_wait = the root event after which the last gather's copies have read d_gather */
    void* d_gather;
    size_t cap_gather;
    hipEvent_t g_done, g_copied, g_wait;
    int g_wait_pending;
    unsigned long long peer_on; /* bit d: peer access to device d enabled from this device */
    /* bhrt_render_frame_ss (supersample.c): device outputs of a host-array frame */
    void* d_ss;
    size_t cap_ss;
} devctx_t;

static _Thread_local devctx_t* g_ctx[BHRT_MAX_DEV];
static _Thread_local bhrt_stats g_stats;
static int g_refill = 0; /* 0: chosen per scene (refill_default) */

/* claim order of this thread's next device camera frames (bhrt_set_claim_order): a device
 * permutation of [0, n) on device g_order_dev, used only by bhrt_render_frame_device calls on
 * that device for frames of exactly n rays (never by the chunks of host-buffer frames) */
static __thread const int* g_order;
static __thread int g_order_n, g_order_dev = -1;
static int current_device(void);
static int env_int(const char* name, int dflt);
int bhrt_set_claim_order(const int* d_order, int n) {
    g_order = NULL;
    g_order_n = 0;
    g_order_dev = -1;
    if (!d_order || n <= 0) return 0;
    const int dev = current_device();
    if (dev < 0) {
        set_err("bhrt_set_claim_order: no current HIP device");
        return -1;
    }
    if (env_int("BHRT_TRUST_CLAIM_ORDER", 0)) { /* the caller guarantees a permutation */
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

void bhrt_set_refill_threshold(int lanes) {
    g_refill = lanes <= 0 ? 0 : (lanes > 64 ? 64 : lanes);
}

/* Refill threshold by the expected ray lifetime. RK4 on a = 0: lifetimes
 * spread over 1..max_steps iterations (C2), so idle lanes are refilled early (8). Otherwise
 * (Kerr: straight-line stages; RKF45: fixed point after a few attempts) rays are short-lived
 * and similar, each refill is an HBM-latency stall, and a wave refills only once drained. */
static int env_int(const char* name, int dflt);
static int refill_default(const bhrt_scene_k* s) {
    const int r = env_int("BHRT_REFILL", 0); /* A/B override */
    if (r >= 1 && r <= 64) return r;
    return (s->method == INTEGRATOR_RK4 && s->spin0) ? 8 : 64;
}

/* Ray queues of k_trace: 2^queue_bits queue heads, queue_stride words apart,
 * and the claim policy. Every claim is a returning device-scope atomic, and claims on ONE word
 * serialise at the memory side (~65 M/s): with one queue, C3 (2 M rays of ~2 iterations) ran
 * at exactly that claim rate. 16 queues: C3 +75%. Where a wave refills only once drained
 * (refill 64: short-lived rays), a claim also takes a block of ids for the next refills
 * (claim_div 1: C3 another +25%, C4 +2%); where lanes are refilled as they finish (C2: rays
 * of 1..1000 iterations) a claim takes exactly the idle lanes -- a block claimed from a stale
 * estimate of the remainder would hold long rays back into the frame's tail (C2 -17%).
 * Same-box sweep: profiles/r02_claim_sweep.txt. BHRT_QUEUES (a power of two),
 * BHRT_QUEUE_STRIDE (words), BHRT_CLAIM_MIN / BHRT_CLAIM_DIV (0 = exactly the idle lanes)
 * override the defaults. */
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

/* Where the trace kernel writes the colour outputs at each ray's exit, from the state in
 * registers (bhrt_colour_in_trace), the separate pass's inputs -- result and hit point -- need
 * not exist on the device. BHRT_FUSE_COLOUR=0 keeps the separate colour pass (A/B). */
static int colour_fused(int method, int has_disk, int spin) {
    return BHRT_COLOUR_IN_TRACE(method, has_disk, spin) && env_int("BHRT_FUSE_COLOUR", 1) != 0;
}

static void claim_policy(bhrt_kparams* kp) {
    int q = env_int("BHRT_QUEUES", 16), bits = 0;
    while (bits < BHRT_MAX_QUEUE_BITS && (2 << bits) <= q) bits++;
    int stride = env_int("BHRT_QUEUE_STRIDE", 32);
    if (stride < 1) stride = 1;
    if (stride > BHRT_QUEUE_STRIDE_MAX) stride = BHRT_QUEUE_STRIDE_MAX;
    int m = env_int("BHRT_CLAIM_MIN", 64), d = env_int("BHRT_CLAIM_DIV", kp->refill >= 64);
    if (m < 64) m = 64;
    if (m > 1 << 16) m = 1 << 16;
    kp->queue_bits = bits;
    kp->queue_stride = stride;
    kp->claim_min = (m + 63) & ~63;
    kp->claim_div = d < 0 ? 0 : d;
}

int bhrt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    const char* cap = getenv("BHRT_MAX_DEVICES");
    if (cap && atoi(cap) > 0 && atoi(cap) < n) n = atoi(cap);
    if (n > BHRT_MAX_DEV) n = BHRT_MAX_DEV;
    return n;
}

static devctx_t* ctx_get(int device) {
    if (device < 0 || device >= BHRT_MAX_DEV) {
        set_err("device %d out of range", device);
        return NULL;
    }
    if (g_ctx[device]) return g_ctx[device];
    if (hipSetDevice(device) != hipSuccess) {
        set_err("hipSetDevice(%d) failed", device);
        return NULL;
    }
    devctx_t* c = (devctx_t*)calloc(1, sizeof *c);
    if (!c) return NULL;
    c->device = device;
    if (hipMalloc((void**)&c->d_ctl, BHRT_RING_BYTES) != hipSuccess ||
        hipHostMalloc((void**)&c->h_ctl,
                      (size_t)BHRT_RING * BHRT_CTL_WORDS * sizeof(unsigned long long), 0) !=
            hipSuccess) {
        set_err("cannot allocate the control blocks on device %d", device);
        free(c);
        return NULL;
    }
    c->ring_dirty = 1; /* zeroed on the GPU by the first launch (ring_order) */
    c->dirty_row = 0;
    c->dirty_rows = BHRT_RING;
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess &&
            khz > 0)
            c->clock_khz = (double)khz;
    }
    /* the harvest's strided D2H copy once here, on the legacy default stream as bhrt_get_stats'
     * harvest does it: a process's first such copy (the runtime's copy kernels loaded, the
     * default stream's queue set up) costs ~6-7 ms, measured as GPU idle time before bench.py's
     * timed frames when the first harvest came there. Synchronous: it waits once, at context
     * creation, for what the caller queued on its default stream. */
    if (hipMemcpy2D(c->h_ctl, BHRT_CTL_WORDS * sizeof(unsigned long long), c->d_ctl,
                    BHRT_SLOT_WORDS * sizeof(unsigned long long),
                    BHRT_CTL_WORDS * sizeof(unsigned long long), 1,
                    hipMemcpyDeviceToHost) != hipSuccess) {
        set_err("cannot read the control blocks on device %d", device);
        free(c);
        return NULL;
    }
    if (hipEventCreateWithFlags(&c->ring_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->nul_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->nul_out, hipEventDisableTiming) != hipSuccess) {
        set_err("hipEventCreate failed");
        free(c);
        return NULL;
    }
    if (hipEventCreate(&c->span_ref) != hipSuccess) {
        set_err("hipEventCreate failed");
        free(c);
        return NULL;
    }
    for (int i = 0; i < 2 * BHRT_RING; i++)
        if (hipEventCreate(&c->evpool[i]) != hipSuccess) {
            set_err("hipEventCreate failed");
            free(c);
            return NULL;
        }
    for (int i = 0; i < BHRT_MAX_CHUNKS; i++)
        if (hipEventCreateWithFlags(&c->chunk_done[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->chunk_copied[i], hipEventDisableTiming) != hipSuccess) {
            set_err("hipEventCreate failed");
            free(c);
            return NULL;
        }
    for (int f = 0; f < BHRT_FRAME_SLOTS; f++)
        for (int i = 0; i < BHRT_MAX_CHUNKS; i++)
            for (int q = -2; q < BHRT_COPY_PARTS; q++)
                if (hipEventCreateWithFlags(q == -2 ? &c->fr[f].done[i]
                                            : q == -1 ? &c->fr[f].copied[i] : &c->fr[f].part[i][q],
                                            hipEventDisableTiming) != hipSuccess) {
                    set_err("hipEventCreate failed");
                    free(c);
                    return NULL;
                }
    g_ctx[device] = c;
    return c;
}

static int ensure(void** p, size_t* cap, size_t need, int pinned);

/* libbhrt's own streams of a context (the default launch stream, the second trace stream and
 * the copy stream of the host-buffer paths), created on first use with c's device current:
 * a caller that only drives the device API on its own streams (bench.py) never creates them,
 * so they take none of the process's hardware queues (GPU_MAX_HW_QUEUES; streams beyond it
 * share a queue, and work on a shared queue runs in order) */
/* One of libbhrt's own streams (device current). Every stream is bound to a hardware queue
 * (GPU_MAX_HW_QUEUES per process, assigned round robin over the process's streams), and work on
 * one queue runs in order: if the two trace streams of a ray batch, or a trace stream and the
 * copy stream, land on one queue, chunk k + 1 cannot fill chunk k's tail and a chunk's download
 * waits for the next chunk's trace. Which queue a plain stream gets depends on how many streams
 * the process made before (torch's: trace_rays_batch ran 144 instead of 200 Mrays/s after two
 * torch streams, profiles/r04/session_p). BHRT_STREAM_QUEUE: 0 = plain non-blocking stream,
 * 1 = the greatest stream priority (default: queues of that priority, which only libbhrt's
 * streams use -- 146 -> 204 Mrays/s in that case, neutral elsewhere, profiles/r04/session_q),
 * 2 = a full CU mask (a queue of its own). */
static int own_stream(hipStream_t* s) {
    const int mode = env_int("BHRT_STREAM_QUEUE", 1);
    if (mode == 1) {
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
            return hipStreamCreateWithPriority(s, hipStreamNonBlocking, hi) == hipSuccess ? 0 : -1;
    } else if (mode == 2) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
            cus > 0 && cus <= 1024) {
            uint32_t mask[32];
            const int words = (cus + 31) / 32;
            for (int i = 0; i < words; i++)
                mask[i] = (i == words - 1 && cus % 32) ? (1u << (cus % 32)) - 1u : 0xffffffffu;
            return hipExtStreamCreateWithCUMask(s, (uint32_t)words, mask) == hipSuccess ? 0 : -1;
        }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess ? 0 : -1;
}

static int ctx_streams(devctx_t* c) {
    if (c->stream && c->stream2 && c->copy) return 0;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != c->device) {
        if (hipSetDevice(c->device) != hipSuccess) {
            set_err("hipSetDevice(%d) failed", c->device);
            return -1;
        }
    }
    if ((!c->stream && own_stream(&c->stream)) || (!c->stream2 && own_stream(&c->stream2)) ||
        (!c->copy && own_stream(&c->copy))) {
        set_err("cannot create libbhrt's streams on device %d", c->device);
        if (cur >= 0 && cur != c->device) (void)hipSetDevice(cur);
        return -1;
    }
    if (cur >= 0 && cur != c->device && hipSetDevice(cur) != hipSuccess) return -1;
    return 0;
}

/* launch scratch of `stream` on this context, at least `bytes` */
static void* stream_scratch(devctx_t* c, hipStream_t stream, size_t bytes);

static int ensure(void** p, size_t* cap, size_t need, int pinned) {
    if (*cap >= need && *p) return 0;
    size_t n = need + need / 4 + 4096;
    if (*p) {
        if (pinned) (void)hipHostFree(*p);
        else (void)hipFree(*p);
        *p = NULL;
        *cap = 0;
    }
    hipError_t e = pinned ? hipHostMalloc(p, n, 0) : hipMalloc(p, n);
    if (e != hipSuccess) {
        set_err("allocation of %zu bytes failed: %s", n, hipGetErrorString(e));
        *p = NULL;
        return -1;
    }
    *cap = n;
    return 0;
}

static void* stream_scratch(devctx_t* c, hipStream_t stream, size_t bytes) {
    int slot = -1;
    for (int i = 0; i < BHRT_SCRATCH_SLOTS; i++)
        if (c->scratch[i].p && c->scratch[i].stream == stream) slot = i;
    if (slot < 0) {
        slot = c->scratch_next;
        c->scratch_next = (c->scratch_next + 1) % BHRT_SCRATCH_SLOTS;
        if (c->scratch[slot].p && hipStreamSynchronize(c->scratch[slot].stream) != hipSuccess) {
            set_err("hipStreamSynchronize failed");
            return NULL;
        }
        c->scratch[slot].stream = stream;
    } else if (c->scratch[slot].cap < bytes &&
               hipStreamSynchronize(stream) != hipSuccess) { /* in use until drained */
        set_err("hipStreamSynchronize failed");
        return NULL;
    }
    if (ensure(&c->scratch[slot].p, &c->scratch[slot].cap, bytes ? bytes : 64, 0)) return NULL;
    return c->scratch[slot].p;
}

/* The control ring is zeroed on the GPU, never with a host sync: after a harvest (ring_dirty)
 * the next launch fills the harvested slots on its own stream before its kernel, and a launch
 * on any other stream in the same cycle first waits for that fill (an event wait; the streams
 * already ordered after it are remembered). Each launch of a cycle takes a slot of the filled
 * range that no earlier launch of the cycle used, so the fill is the only ordering a slot
 * needs. (Round 5 zeroed the ring on the legacy null stream and synchronised it: a host stall
 * behind every piece of default-stream work of the caller, once per BHRT_RING launches.) */
static int ring_order(devctx_t* c, hipStream_t st) {
    if (c->ring_dirty) {
        HIP_TRY(hipMemsetAsync(c->d_ctl + (size_t)c->dirty_row * BHRT_SLOT_WORDS, 0,
                               (size_t)c->dirty_rows * BHRT_SLOT_WORDS * sizeof(unsigned long long),
                               st));
        HIP_TRY(hipEventRecord(c->ring_ev, st));
        c->ring_dirty = 0;
        c->ring_ok[0] = st;
        c->n_ring_ok = 1;
        return 0;
    }
    for (int i = 0; i < c->n_ring_ok; i++)
        if (c->ring_ok[i] == st) return 0;
    HIP_TRY(hipStreamWaitEvent(st, c->ring_ev, 0));
    if (c->n_ring_ok < BHRT_RING_STREAMS) c->ring_ok[c->n_ring_ok++] = st;
    return 0;
}

/* Wait for the pending launches and read their counters; fold them into g_stats (fold = 0
 * drops them unread, without the per-launch event timing: a caller resetting the statistics
 * right before a timed region must not leave the GPU idle for the ~0.2 ms per launch that the
 * event queries take, bench.py). Either way a launch whose redo pass was left out (the host
 * proved no ray can need it, origin_no_evict) must not have handed a ray over: if one did, the
 * proof was wrong for that scene, the ray's outputs hold RAY_ERROR (k_trace), and this
 * returns -1 with the count in bhrt_last_error.
 * The counters are read on `st`: the stream of the launch that found the ring full (its earlier
 * work precedes that launch anyway, and the caller keeps it alive), or with st = NULL -- a
 * bhrt_get_stats call, itself a synchronisation point -- a synchronous copy on the legacy
 * default stream. Round 6 first read them on a control stream of libbhrt's own: one hardware
 * queue more in the process, created before the caller's render streams had theirs, cost C4's
 * 8-GPU shard 15% (profiles/r06/ab_control_stream.txt).
 * `count`: how many of the oldest pending launches. A launch that finds the ring full harvests
 * its older half only (BHRT_RING / 2 launches, long finished when frames are in flight), so the
 * GPU keeps the newer half's frames while the host reads; it then reuses the freed half. The
 * slots of the pending launches are consecutive, the ring alternates halves (a full harvest
 * restarts it at slot 0), and the older half never wraps. bhrt_get_stats harvests everything. */
static int harvest(devctx_t* c, int fold, hipStream_t st, int count) {
    if (count > c->npend) count = c->npend;
    if (count <= 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < count; i++) HIP_TRY(hipEventSynchronize(c->pend[i].ev1));
    const int full = count == c->npend;
    const int row = full ? 0 : c->pend[0].slot, rows = full ? BHRT_RING : count;
    if (row + rows > BHRT_RING) {
        set_err("internal: control ring range %d+%d", row, rows);
        return -1;
    }
    if (st) {
        HIP_TRY(hipMemcpy2DAsync(c->h_ctl + (size_t)row * BHRT_CTL_WORDS,
                                 BHRT_CTL_WORDS * sizeof(unsigned long long),
                                 c->d_ctl + (size_t)row * BHRT_SLOT_WORDS,
                                 BHRT_SLOT_WORDS * sizeof(unsigned long long),
                                 BHRT_CTL_WORDS * sizeof(unsigned long long), rows,
                                 hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        HIP_TRY(hipMemcpy2D(c->h_ctl + (size_t)row * BHRT_CTL_WORDS,
                            BHRT_CTL_WORDS * sizeof(unsigned long long),
                            c->d_ctl + (size_t)row * BHRT_SLOT_WORDS,
                            BHRT_SLOT_WORDS * sizeof(unsigned long long),
                            BHRT_CTL_WORDS * sizeof(unsigned long long), rows,
                            hipMemcpyDeviceToHost));
    }
    /* the harvested slots are free again: the next launch zeroes them and takes them first */
    c->ring_dirty = 1;
    c->dirty_row = row;
    c->dirty_rows = rows;
    if (full) c->next_slot = 0;
    unsigned long long lost = 0;
    for (int i = 0; i < count; i++) {
        const unsigned long long* w = c->h_ctl + c->pend[i].slot * BHRT_CTL_WORDS;
        if (!c->pend[i].redo) lost += w[6];
        if (!fold) continue;
        float t0 = 0.f, t1 = 0.f, dt = 0.f; /* start and end relative to span_ref (ms) */
        HIP_TRY(hipEventElapsedTime(&t0, c->span_ref, c->pend[i].ev0));
        HIP_TRY(hipEventElapsedTime(&t1, c->span_ref, c->pend[i].ev1));
        /* the launch's own duration from its own pair: a difference of two values relative to
         * span_ref would lose precision as span_ref ages (float ms) */
        HIP_TRY(hipEventElapsedTime(&dt, c->pend[i].ev0, c->pend[i].ev1));
        if (t0 < c->span_lo) c->span_lo = t0;
        if (t1 > c->span_hi) c->span_hi = t1;
        g_stats.rays += w[1];
        g_stats.iterations += w[2];
        if (c->pend[i].untested) g_stats.attempts_untested += w[2];
        g_stats.stages_full += w[3];
        g_stats.stages_far += w[4];
        g_stats.stages_kerr += w[5];
        g_stats.rays_redone += w[6];
        g_stats.redo_launches += (uint64_t)c->pend[i].redo;
        g_stats.launches += 1;
        g_stats.kernel_ms += dt;
        /* the execution window: earliest wave start (stored complemented) to the latest end */
        const unsigned long long t_end = w[9] > w[10] ? w[9] : w[10];
        if (c->clock_khz > 0.0 && w[8] != 0 && t_end >= ~w[8]) {
            const double ms = (double)(t_end - ~w[8]) / c->clock_khz;
            g_stats.frame_ms += ms;
            if (ms > g_stats.frame_ms_max) g_stats.frame_ms_max = ms;
            g_stats.frames_timed += 1;
        }
    }
    c->npend -= count;
    if (c->npend > 0) memmove(c->pend, c->pend + count, (size_t)c->npend * sizeof c->pend[0]);
    if (lost) {
        set_err("%llu ray(s) needed the large-argument redo pass that the host had proved "
                "unnecessary and left out: their outputs hold RAY_ERROR (BHRT_SKIP_REDO=0 "
                "always runs the pass)", lost);
        return -1;
    }
    return 0;
}

int bhrt_get_stats(bhrt_stats* out, int reset) {
    int rc = 0;
    double span = 0.0;
    int cur = -1;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < BHRT_MAX_DEV; d++) {
        devctx_t* c = g_ctx[d];
        if (!c) continue;
        if (harvest(c, out != NULL || !reset, NULL, c->npend) != 0) rc = -1;
        if (c->span_on && c->span_hi > c->span_lo) span += c->span_hi - c->span_lo;
        if (reset) c->span_on = 0;
    }
    if (cur >= 0) (void)hipSetDevice(cur); /* (harvest makes each context's device current) */
    g_stats.span_ms = span;
    if (out) *out = g_stats;
    if (reset) memset(&g_stats, 0, sizeof g_stats);
    return rc;
}

/* ======================================================================================= */
/* launch plumbing                                                                          */
/* ======================================================================================= */
/* The disk test's inner <= sqrt(qx^2+qy^2) <= outer (raytracer.c:190-191) without the square
 * root: sqrt is correctly rounded and monotone, so {s : RN(sqrt(s)) >= inner} = {s >= lo} and
 * {s : RN(sqrt(s)) <= outer} = {s <= hi} for the thresholds found here by stepping from the
 * rounded square (a few ulps). NaN bounds keep the comparisons false, as in the reference. */
static double sqrt_lower_bound(double inner) {
    if (isnan(inner)) return NAN;
    if (inner <= 0.0) return -INFINITY;
    double s = inner * inner;
    while (s > 0.0 && sqrt(nextafter(s, 0.0)) >= inner) s = nextafter(s, 0.0);
    while (sqrt(s) < inner) s = nextafter(s, INFINITY);
    return s;
}

static double sqrt_upper_bound(double outer) {
    if (isnan(outer)) return NAN;
    if (outer < 0.0) return -INFINITY;
    if (isinf(outer)) return INFINITY;
    double s = outer * outer;
    while (sqrt(s) > outer) s = nextafter(s, 0.0);
    while (!isinf(s) && sqrt(nextafter(s, INFINITY)) <= outer) s = nextafter(s, INFINITY);
    return s;
}

/* Whether every state the trace loop can reach from an initial state within 2^40 stays below
 * 2^400 for max_steps steps with the far-field branch taking part (geodesic.hip
 * repair_at_refill: the far-field instantiations then run the state recovery once per ray and
 * the division-free RKF45 accept test). Stage accelerations are clamped to 10, zero, or -- in
 * the far-field branch, only where y0 > 15 rs -- y5 * 2M / y0^2 with a factor below
 * C = 2M / (15 rs)^2. With h the largest step size, S = 18 >= the largest stage weight sum of
 * RK4 (1) and RKF45 (17.4), W = 1.5 >= the final combination's (RK4 1, RKF45 1.4) and q = h S C
 * < 1/2, a stage velocity is at most 2 (V + 10 h S) for velocities V at the step's start, so
 * V' <= g V + a with g = 1 + 2 h W C, a = 20 h W: V_N <= g^N (V_0 + N a); the position moves
 * by at most 2 h W (V + 10 h S) per step. */
static int far_bounded(const bhrt_scene_k* s) {
    if (s->max_steps <= 0) return 1;
    if (!(s->two_m >= 0.0) || !(s->rs_x15 > 0.0 || s->two_m == 0.0)) return 0;
    const double C = s->two_m == 0.0 ? 0.0 : s->two_m / (s->rs_x15 * s->rs_x15) * (1.0 + 1e-9);
    const double h = fmax(fmax(fabs(s->h_2_5), fabs(s->h_5)), fmax(fabs(s->h_15), fabs(s->h_far)));
    const double S = 18.0, W = 1.5, N = (double)s->max_steps;
    if (!isfinite(C) || !isfinite(h) || !(h * S * C < 0.5)) return 0;
    const double logv = log2(0x1p40 + N * 20.0 * h * W) + N * log1p(2.0 * h * W * C) / log(2.0);
    const double logp = log2(0x1p40 + N * 2.0 * h * W * (exp2(fmin(logv, 1000.0)) + 10.0 * h * S));
    return logv <= 400.0 && logp <= 400.0;
}

/* Whether no ray that starts at this origin can be handed to the redo pass (geodesic.hip k_trace:
 * a finite sincos argument |x| >= 2^20, a far-field state the host could not prove bounded, or
 * -- on the zero-acceleration Kerr paths -- |state[5]| >= rot_vmax). Then the redo launch is
 * left out (launch_trace_pair): one dispatch less per frame, and a frame's completion no longer
 * waits behind the next frame's persistent workgroups for a wave slot.
 * The live state is (t, r, theta, phi, tdot, rdot); ray_derivatives reads it shifted, so the
 * derivatives of components 0..2 are components 3..5 ("velocities" V) and those of 3..5 are
 * accelerations: clamped to 10, zero (Kerr), or -- far-field branch, only where y0 > 15 rs --
 * y5 * 2M / y0^2 with a factor below C = 2M / (15 rs)^2. With h the largest step size, S the
 * largest stage weight sum (RK4 1, RKF45 17.4 -> 18) and W the final combination's (RK4 1,
 * RKF45 1.4 -> 1.5): without the far-field branch a stage velocity is at most V + 10 h S, a step
 * moves V by at most 10 h W and the positions P by at most h W (V + 10 h S); with it (q = h S C
 * < 1/2) a stage velocity is at most 2 (V + 10 h S), V' <= g V + 20 h W with g = 1 + 2 h W C,
 * and P moves by at most 2 h W (V + 10 h S) (far_bounded's argument). The initial state: t = 0,
 * r, theta, phi of the origin, rdot = n.e_r <= 1 and tdot^2 <= (|g_rr| + (g_hh / r^2)(1 + 1 /
 * sin^2 theta)) / |g_tt| (n a unit vector; its components on the orthonormal e_theta, e_phi
 * give theta-dot = n.e_theta / r, phi-dot = n.e_phi / (r sin theta)). Every sincos argument
 * of the loop is a (stage) value of components 1..3, so a bound below 2^20 proves the claim. */
static int origin_no_evict(const bhrt_scene_k* s, double r, double th, double ph, double st,
                           int st_tiny, double g_tt, double g_rr, double g_hh, int far) {
    if (s->max_steps <= 0) return 1;
    const int rkf = s->method == INTEGRATOR_RKF45;
    if (!rkf && s->method != INTEGRATOR_RK4) return 1; /* (no-op integrators: no step at all) */
    if (!s->spin0 && !far) /* the rotation paths: no sincos in the loop; |rdot| <= 1 + 2^-50 */
        return s->rot_vmax > 1.001;
    if (far && !s->far_bounded) return 0;
    if (!(isfinite(r) && isfinite(th) && isfinite(ph) && isfinite(g_tt) && isfinite(g_rr) &&
          isfinite(g_hh) && g_tt != 0.0 && r != 0.0))
        return 0;
    const double h = fmax(fmax(fabs(s->h_2_5), fabs(s->h_5)), fmax(fabs(s->h_15), fabs(s->h_far)));
    if (!isfinite(h)) return 0;
    const double S = rkf ? 18.0 : 1.0, W = rkf ? 1.5 : 1.0, N = (double)s->max_steps;
    const double sl = 1.0 + 1e-6; /* slack for the rounding of the set-up's products */
    const double inv_st2 = st_tiny ? 0.0 : 1.0 / (st * st);
    if (!isfinite(inv_st2)) return 0;
    const double vt2 = (fabs(g_rr) + fabs(g_hh) / (r * r) * (1.0 + inv_st2)) / fabs(g_tt);
    const double V0 = fmax(fmax(fabs(ph), sqrt(vt2) * sl), sl);
    const double P0 = fmax(fabs(r), fabs(th));
    double V, P, B;
    if (!far || s->two_m == 0.0) {
        V = V0 + N * 10.0 * h * W;
        P = P0 + N * h * W * (V + 10.0 * h * S);
        B = fmax(P + h * S * (V + 10.0 * h * S), V + 10.0 * h * S);
    } else {
        const double C = s->two_m / (s->rs_x15 * s->rs_x15) * (1.0 + 1e-9);
        if (!isfinite(C) || !(h * S * C < 0.5)) return 0;
        const double lg = N * log1p(2.0 * h * W * C);
        if (!(lg < 40.0)) return 0;
        V = exp(lg) * (V0 + N * 20.0 * h * W);
        P = P0 + N * 2.0 * h * W * (V + 10.0 * h * S);
        B = fmax(P + 2.0 * h * S * (V + 10.0 * h * S), 2.0 * (V + 10.0 * h * S));
    }
    return isfinite(B) && B * sl < 1048576.0;
}

static int fill_scene(bhrt_kparams* kp, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                      const SimulationConfig* cfg, IntegrationMethod method, int flags) {
    memset(kp, 0, sizeof *kp);
    bhrt_scene_k* s = &kp->sc;
    const double rs = bh->schwarzschild_radius, dt = cfg->time_step;
    /* the products the reference forms inline (raytracer.c:65-130, 465, 556-571, 652) */
    s->M = bh->mass;
    s->rs = rs;
    s->two_m = 2.0 * bh->mass;
    s->rs_x1_5 = rs * 1.5;
    s->rs_x1_05 = rs * 1.05;
    s->rs_x2_5 = rs * 2.5;
    s->rs_x5 = rs * 5.0;
    s->rs_x15 = rs * 15.0;
    s->rs_eps = rs + BH_EPSILON;
    /* the schedule's candidates with fmin(h, 0.1) applied (raytracer.c:556-571) */
    s->h_2_5 = fmin(dt * 0.001, 0.1);
    s->h_5 = fmin(dt * 0.01, 0.1);
    s->h_15 = fmin(dt * 0.1, 0.1);
    s->h_far = fmin(dt, 0.1);
    /* the r interval each step size holds on (geodesic.hip ray_iterate caches the size and its
     * interval per ray): the chain picks h_2_5 for r < t3, else h_5 for r < t2, else h_15 for
     * r < t1, else h_far -- for any order of the thresholds */
    {
        const double t1 = s->rs_x15, t2 = s->rs_x5, t3 = s->rs_x2_5;
        s->h_lo[3] = -INFINITY;
        s->h_hi[3] = t3;
        s->h_lo[2] = t3;
        s->h_hi[2] = t2;
        s->h_lo[1] = fmax(t2, t3);
        s->h_hi[1] = t1;
        s->h_lo[0] = fmax(t1, fmax(t2, t3));
        s->h_hi[0] = INFINITY;
    }
    {
        /* a step's nominal increment of state[2] is h * (a weighted sum of the constant
         * state[5] whose weights' magnitudes add up to <= 1.36, RKF45's 5th order; RK4 1) */
        const double hmax = fmax(fmax(fabs(s->h_2_5), fabs(s->h_5)), fmax(fabs(s->h_15), fabs(s->h_far)));
        s->rot_vmax = hmax > 0.0 ? 0.78 / (hmax * 1.4) : INFINITY; /* 0.78 < pi/4 */
        if (!(s->rot_vmax >= 0.0)) s->rot_vmax = 0.0;              /* (NaN / Inf step sizes) */
    }
    s->max_dist = cfg->max_ray_distance;
    s->tol = cfg->tolerance;
    s->max_steps = cfg->max_integration_steps;
    s->method = (int)method;
    s->flags = flags;
    s->spin0 = bh->spin == 0.0;
    s->far_bounded = far_bounded(s);
    /* on the zero-acceleration paths an attempt's error is rounding alone, < 6e-15 of its scale
     * (proof at geodesic.hip rkf45_attempt): every attempt is accepted for tol >= 2^-30.
     * BHRT_ACCEPT_ALL=0 keeps the test (A/B) */
    s->accept_all = method == INTEGRATOR_RKF45 && s->tol >= 0x1p-30 && s->tol <= 0x1p300 &&
                    isfinite(s->h_2_5) && isfinite(s->h_5) && isfinite(s->h_15) &&
                    isfinite(s->h_far) && env_int("BHRT_ACCEPT_ALL", 1) != 0;
    s->has_disk = dk != NULL;
    if (dk) {
        s->disk_in = dk->inner_radius;
        s->disk_out = dk->outer_radius;
        s->disk_tscale = dk->temperature_scale;
        s->disk_in_sq = sqrt_lower_bound(dk->inner_radius);
        s->disk_out_sq = sqrt_upper_bound(dk->outer_radius);
    }
    kp->refill = g_refill ? g_refill : refill_default(s);
    claim_policy(kp);
    kp->colour_fused = colour_fused((int)method, dk != NULL, bh->spin != 0.0);
    kp->skip_redo = env_int("BHRT_SKIP_REDO", 1) != 0;
    kp->block_lanes = env_int("BHRT_TRACE_BLOCK", 256);
    kp->grid_div = env_int("BHRT_GRID_DIV", 0);
    kp->grid_blocks = env_int("BHRT_GRID_BLOCKS", 0);
    kp->min_tiles = env_int("BHRT_MIN_TILES", 10);
    kp->cam.rows.row_block = 1;
    kp->cam.rows.num_shards = 1;
    return 0;
}

/* camera basis exactly as calculate_ray_direction forms it (raytracer.c:1013-1028), and
 * integrate_photon_path's origin-only set-up (raytracer.c:355-466, spacetime.c:15-33,
 * 201-237): every camera ray shares the origin, so its spherical coordinates, their sin/cos
 * and the metric there are computed once, here, with the same libm calls as the reference. */
static void fill_origin(bhrt_kparams* kp, const Vector3D* origin);
static void fill_camera(bhrt_kparams* kp, const bhrt_camera* cam, int W, int H) {
    bhrt_camera_k* k = &kp->cam;
    double aspect = (double)W / (double)H;
    Vector3D fwd = vector3D_normalize(cam->direction);
    Vector3D right = vector3D_normalize(vector3D_cross(fwd, cam->up));
    Vector3D up = vector3D_cross(right, fwd);
    double fov_radians = cam->fov_deg * BH_PI / 180.0;
    double plane_h = 2.0 * tan(fov_radians / 2.0);
    kp->src = BHRT_SRC_CAMERA;
    k->fwd[0] = fwd.x; k->fwd[1] = fwd.y; k->fwd[2] = fwd.z;
    k->right[0] = right.x; k->right[1] = right.y; k->right[2] = right.z;
    k->up[0] = up.x; k->up[1] = up.y; k->up[2] = up.z;
    k->plane_h = plane_h;
    k->plane_w = plane_h * aspect;
    k->off_x = cam->use_offset ? cam->offset_x : 0.5;
    k->off_y = cam->use_offset ? cam->offset_y : 0.5;
    k->width = W;
    k->height = H;
    k->inv_width = 1.0 / (double)W;
    k->inv_block = 1.0 / (double)k->rows.row_block;
    fill_origin(kp, &cam->position);
}

/* integrate_photon_path's origin-only set-up for rays that share `origin` (a camera frame, or
 * a ray array whose every origin is this one: shared_origin) */
static void fill_origin(bhrt_kparams* kp, const Vector3D* origin) {
    bhrt_camera_k* k = &kp->cam;
    k->pos[0] = origin->x;
    k->pos[1] = origin->y;
    k->pos[2] = origin->z;
    Vector3D sph;
    cartesian_to_spherical(origin, &sph);
    double r = sph.x, th = sph.y, ph = sph.z;
    double st = sin(th), ct = cos(th), sp = sin(ph), cp = cos(ph);
    k->r0 = r;
    k->th0 = th;
    k->ph0 = ph;
    k->st_cp = st * cp;
    k->st_sp = st * sp;
    k->ct = ct;
    k->ct_cp = ct * cp;
    k->ct_sp = ct * sp;
    k->st = st;
    k->neg_sp = -sp;
    k->cp = cp;
    k->r_st = r * st;
    k->st_tiny = fabs(st) < BH_EPSILON;
    SchwarzschildMetric m = calculate_schwarzschild_metric(r, &(BlackHoleParams){
        .schwarzschild_radius = kp->sc.rs});
    k->g_tt = m.g_tt;
    k->g_rr = m.g_rr;
    k->g_hh = m.g_thth;
    Vector3D p0;
    spherical_to_cartesian(&sph, &p0);
    k->p0[0] = p0.x;
    k->p0[1] = p0.y;
    k->p0[2] = p0.z;
    k->use_approx = r > kp->sc.rs_x15;
    /* the carried sin/cos of the origin's state angles start from the
     * reference's own libm values: state[2..3] = (th0, ph0) are st, ct, sp, cp above, and
     * state[1] = r0 is read as an angle by ray_derivatives */
    k->sp = sp;
    k->s_r0 = sin(r);
    k->c_r0 = cos(r);
    /* BHRT_ASSUME_NO_EVICT=1 (tests only): take the proof as given, so that a scene that does
     * evict shows what a wrong proof would do -- RAY_ERROR outputs and a harvest error */
    kp->no_evict = env_int("BHRT_ASSUME_NO_EVICT", 0) ||
                   origin_no_evict(&kp->sc, r, th, ph, st, k->st_tiny, m.g_tt, m.g_rr, m.g_thth,
                                   k->use_approx);
}

/* one timed kernel launch on `stream` (the context's own if NULL) with a control block of the
 * ring: the trace kernel (fn NULL), or fn(kp, arg, stream, ev0, ev1) -- a launcher with
 * bhrt_launch_trace's contract that another host file names (bhrt_hook_launch) */
static int launch_fn(devctx_t* c, bhrt_kparams* kp, hipStream_t stream, bhrt_launch_fn fn,
                     const void* arg) {
    if (kp->n <= 0) return 0;
    if (!stream) {
        if (ctx_streams(c)) return -1;
        stream = c->stream;
    }
    /* the redo list follows the initial-state table (one extra field of the allocation) */
    if (kp->init) kp->redo = (int*)(kp->init + (size_t)BHRT_INIT_FIELDS * (size_t)kp->n);
    if (c->npend == BHRT_RING &&
        harvest(c, 1, stream, env_int("BHRT_HARVEST_ALL", 0) ? BHRT_RING : BHRT_RING / 2) != 0)
        return -1;
    if (ring_order(c, stream)) return -1;
    int slot = c->next_slot;
    c->next_slot = (c->next_slot + 1) % BHRT_RING;
    kp->ctl = c->d_ctl + (size_t)slot * BHRT_SLOT_WORDS;
    kp->qhead = kp->ctl + BHRT_QHEAD_OFF;
    kp->diag_slot = slot;
    /* (the slot was zeroed when it was last harvested, or at the context's creation) */
    if (env_int("BHRT_LAUNCH_MEMSET", 0))  /* A/B: the per-launch fill kernel of round 4 */
        HIP_TRY(hipMemsetAsync(kp->ctl, 0,
                               (BHRT_QHEAD_OFF + ((size_t)kp->queue_stride << kp->queue_bits)) *
                                   sizeof(unsigned long long),
                               stream));
    if (!c->span_on) {
        HIP_TRY(hipEventRecord(c->span_ref, stream));
        c->span_on = 1;
        c->span_lo = 1e300;
        c->span_hi = -1e300;
    }
    pending_t* p = &c->pend[c->npend];
    p->slot = slot;
    p->redo = fn ? 0 : !(kp->skip_redo && kp->no_evict); /* (fn: no redo pass, and no evictions) */
    p->untested = fn ? 0 : bhrt_trace_untested(kp);
    p->ev0 = c->evpool[2 * slot]; /* (per slot: a slot has one pending launch at most) */
    p->ev1 = c->evpool[2 * slot + 1];
    int e = fn ? fn(kp, arg, (void*)stream, (void*)p->ev0, (void*)p->ev1)
               : bhrt_launch_trace(kp, (void*)stream, (void*)p->ev0, (void*)p->ev1);
    if (e != 0) {
        set_err("%s kernel launch failed: %s", fn ? "path" : "trace",
                hipGetErrorString((hipError_t)e));
        return -1;
    }
    c->npend++;
    return 0;
}

static int launch(devctx_t* c, bhrt_kparams* kp, hipStream_t stream) {
    return launch_fn(c, kp, stream, NULL, NULL);
}

static int current_device(void) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return -1;
    return d;
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

static int check_scene(const BlackHoleParams* bh, const SimulationConfig* cfg) {
    if (!bh || !cfg) {
        set_err("blackhole and config must not be NULL");
        return -1;
    }
    return 0;
}

/* the colour pass (rgb and/or the display fields) reads result and the hit point */
static int colour_args_bad(const bhrt_frame_soa* out, int method, int has_disk, int spin) {
    if ((out->rgb_r || out->rgb_g || out->rgb_b) && !(out->rgb_r && out->rgb_g && out->rgb_b)) {
        set_err("rgb output needs all of rgb_r/g/b");
        return 1;
    }
    if ((out->rgb_r || out->rgba32f || out->rgba8) && !colour_fused(method, has_disk, spin) &&
        (!out->result || !out->hit_x || !out->hit_y)) {
        set_err("colour outputs need result and hit_x/hit_y (separate colour pass)");
        return 1;
    }
    return 0;
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
    if (env_int("BHRT_TILES", 1) == 0) return;
    for (int i = 0; i < 3; i++) {
        const int tw = 1 << shape[i][0], th = 1 << shape[i][1];
        if (W % tw == 0 && nrows % th == 0) {
            k->tile_w_log2 = shape[i][0];
            k->tile_h_log2 = shape[i][1];
            k->tiles_per_row = W / tw;
            k->inv_tiles_per_row = 1.0 / (double)k->tiles_per_row;
            k->ntiles = k->tiles_per_row * (nrows / th);
            k->tile_stride = 0;
            if (env_int("BHRT_TILE_SCATTER", 0) && k->ntiles > 2) {
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

/* use_order: whether the thread's claim order (bhrt_set_claim_order) may apply -- the public
 * device API only; the chunks of host-buffer frames always take the default order */
static int render_frame_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                               const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                               const bhrt_rows* rows, IntegrationMethod method, int flags,
                               const bhrt_frame_soa* out, void* stream, int use_order) {
    if (check_scene(bh, cfg) || !cam || !out || W <= 0 || H <= 0) {
        if (!g_err[0]) set_err("invalid argument");
        return -1;
    }
    int nrows = bhrt_shard_rows(H, rows);
    if (nrows < 0 || (long)nrows * W > 0x7fffffffL) {
        set_err("invalid row sharding or frame too large (%d x %d)", W, H);
        return -1;
    }
    int dev = current_device();
    devctx_t* c = ctx_get(dev);
    if (!c) return -1;
    if (colour_args_bad(out, (int)method, dk != NULL, bh->spin != 0.0)) return -1;
    if (!stream && ctx_streams(c)) return -1;
    void* scratch = stream_scratch(c, stream ? (hipStream_t)stream : c->stream,
                                   (size_t)(BHRT_INIT_FIELDS + 1) * sizeof(double) *
                                       (size_t)nrows * (size_t)W);
    if (!scratch) return -1;
    bhrt_kparams kp;
    fill_scene(&kp, bh, dk, cfg, method, flags);
    fill_camera(&kp, cam, W, H);
    if (rows && rows->num_shards > 1) {
        kp.cam.rows = *rows;
        kp.cam.inv_block = 1.0 / (double)rows->row_block;
    }
    kp.n = nrows * W;
    kp.init = (double*)scratch;
    kp.out = *out;
    if (use_order && g_order && g_order_n == kp.n && g_order_dev == dev) kp.order = g_order;
    else if (method == INTEGRATOR_RK4) claim_tiles(&kp.cam, W, nrows);
    return launch(c, &kp, (hipStream_t)stream);
}

/* A NULL hip_stream in the device API means what it means for a HIP launch: ordered after
 * every piece of work the caller queued on the legacy default stream (a hipMemset or a torch
 * fill of the outputs) and before everything queued there afterwards -- while the kernels
 * still run on libbhrt's own high-priority stream (own_stream: its own hardware queue). Two
 * event hops per call, no host sync: the default stream -> libbhrt's stream before the launch
 * (null_fence(c, 0)) and back after it (null_fence(c, 1)). Round 5 launched NULL calls on
 * libbhrt's non-blocking stream with no ordering at all, and a torch fill still queued behind
 * the trace kernel overwrote 3.37 M of 4.15 M rays of a frame;
 * BHRT_NULL_STREAM=unordered keeps that behaviour as an explicit opt-in. */
static int null_unordered(void) {
    const char* e = getenv("BHRT_NULL_STREAM");
    return e && strcmp(e, "unordered") == 0;
}

static int null_fence(devctx_t* c, int after) {
    if (after) {
        HIP_TRY(hipEventRecord(c->nul_out, c->stream));
        HIP_TRY(hipStreamWaitEvent((hipStream_t)0, c->nul_out, 0));
    } else {
        HIP_TRY(hipEventRecord(c->nul_in, (hipStream_t)0));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->nul_in, 0));
    }
    return 0;
}

/* the current device's context with libbhrt's streams, for a NULL-stream call */
static devctx_t* null_ctx(void) {
    devctx_t* c = ctx_get(current_device());
    return c && ctx_streams(c) == 0 ? c : NULL;
}

int bhrt_render_frame_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                             const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                             const bhrt_rows* rows, IntegrationMethod method, int flags,
                             const bhrt_frame_soa* out, void* stream) {
    if (stream || null_unordered())
        return render_frame_device(bh, dk, cfg, cam, W, H, rows, method, flags, out, stream, 1);
    devctx_t* c = null_ctx();
    if (!c || null_fence(c, 0)) return -1;
    const int rc =
        render_frame_device(bh, dk, cfg, cam, W, H, rows, method, flags, out, c->stream, 1);
    return null_fence(c, 1) ? -1 : rc;
}

/* origin: non-NULL when the host knows every ray starts at *origin (shared_origin): the
 * origin's set-up is then done once here, as for a camera frame, and the trace kernel sets each
 * ray up from its direction alone (no k_init table). The rays are d_rays (AoS), or -- with an
 * origin only -- d_rays NULL and d_dirs their packed directions (3 doubles per ray: half the
 * upload of trace_rays_batch's chunks). */
static int trace_rays_device(const Ray* d_rays, const double* d_dirs, int n,
                             const BlackHoleParams* bh, const AccretionDiskParams* dk,
                             const SimulationConfig* cfg, IntegrationMethod method, int flags,
                             const bhrt_frame_soa* out, void* stream, const Vector3D* origin) {
    if (check_scene(bh, cfg) || !(d_rays || (d_dirs && origin)) || !out || n < 0) {
        if (!g_err[0]) set_err("invalid argument");
        return -1;
    }
    if (colour_args_bad(out, (int)method, dk != NULL, bh->spin != 0.0)) return -1;
    devctx_t* c = ctx_get(current_device());
    if (!c) return -1;
    if (!stream && ctx_streams(c)) return -1;
    void* scratch = stream_scratch(c, stream ? (hipStream_t)stream : c->stream,
                                   (size_t)(BHRT_INIT_FIELDS + 1) * sizeof(double) * (size_t)n);
    if (!scratch) return -1;
    bhrt_kparams kp;
    fill_scene(&kp, bh, dk, cfg, method, flags);
    kp.src = BHRT_SRC_RAYS;
    kp.rays = d_rays;
    kp.init = (double*)scratch;
    kp.n = n;
    kp.out = *out;
    if (origin && (env_int("BHRT_SHARED_ORIGIN", 1) || !d_rays)) {
        fill_origin(&kp, origin);
        kp.rays_shared = 1;
        kp.dirs = d_rays ? &d_rays[0].direction.x : d_dirs;
        kp.dir_stride = d_rays ? (int)(sizeof(Ray) / sizeof(double)) : 3;
    }
    return launch(c, &kp, (hipStream_t)stream);
}

int bhrt_trace_rays_device(const Ray* d_rays, int n, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg,
                           IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                           void* stream) {
    if (stream || null_unordered())
        return trace_rays_device(d_rays, NULL, n, bh, dk, cfg, method, flags, out, stream, NULL);
    devctx_t* c = null_ctx(); /* NULL stream: ordered like the legacy default stream */
    if (!c || null_fence(c, 0)) return -1;
    const int rc =
        trace_rays_device(d_rays, NULL, n, bh, dk, cfg, method, flags, out, c->stream, NULL);
    return null_fence(c, 1) ? -1 : rc;
}

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

/* ---- host-buffer paths: device SoA block <-> caller SoA ---- */
static const size_t k_fsize[BHRT_NFIELDS] = {4, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 16, 4};

static void** soa_slot(bhrt_frame_soa* s, int f) { return ((void**)s) + f; }

/* the fields a device SoA needs for the fields `want_in` requests */
static bhrt_frame_soa device_fields(const bhrt_frame_soa* want_in, int method, int has_disk,
                                    int spin) {
    bhrt_frame_soa want_buf = *want_in;
    if (want_buf.rgb_r || want_buf.rgb_g || want_buf.rgb_b) /* written together */
        want_buf.rgb_r = want_buf.rgb_g = want_buf.rgb_b = (double*)1;
    if ((want_buf.rgb_r || want_buf.rgba32f || want_buf.rgba8) &&
        !colour_fused(method, has_disk, spin)) {
        /* the separate colour pass reads these */
        if (!want_buf.result) want_buf.result = (int32_t*)1;
        if (!want_buf.hit_x) want_buf.hit_x = (double*)1;
        if (!want_buf.hit_y) want_buf.hit_y = (double*)1;
    }
    return want_buf;
}

static size_t soa_bytes(const bhrt_frame_soa* fields, long n) {
    size_t bytes = 0;
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (*soa_slot((bhrt_frame_soa*)fields, f)) bytes += ((k_fsize[f] * n + 255) / 256) * 256;
    return bytes;
}

/* point dev's fields at consecutive 256-byte-aligned arrays of n elements from *p */
static void soa_carve(char** p, const bhrt_frame_soa* fields, long n, bhrt_frame_soa* dev) {
    memset(dev, 0, sizeof *dev);
    for (int f = 0; f < BHRT_NFIELDS; f++)
        if (*soa_slot((bhrt_frame_soa*)fields, f)) {
            *soa_slot(dev, f) = *p;
            *p += ((k_fsize[f] * n + 255) / 256) * 256;
        }
}

/* carve a device SoA for n rays out of c->d_soa, for the fields `want` requests */
static int device_soa(devctx_t* c, long n, const bhrt_frame_soa* want_in, int method,
                      int has_disk, int spin, bhrt_frame_soa* dev) {
    const bhrt_frame_soa fields = device_fields(want_in, method, has_disk, spin);
    const size_t bytes = soa_bytes(&fields, n);
    if (ensure(&c->d_soa, &c->cap_soa, bytes ? bytes : 256, 0)) return -1;
    char* p = (char*)c->d_soa;
    soa_carve(&p, &fields, n, dev);
    return 0;
}

typedef struct {
    devctx_t* c;
    bhrt_frame_soa dev;
    long n;
} shard_job;

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
static int host_threads(void) {
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
    const int nthreads = host_threads();
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
    if (ctx_streams(c)) return -1;
    const size_t bytes = wanted_bytes(j, host);
    if (ensure(&c->h_stage, &c->cap_stage, bytes ? bytes : 64, 1)) return -1;
    if (readback_issue(j, host, (char*)c->h_stage, c->stream, NULL, NULL, NULL)) return -1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    readback_finish(j, host, (const char*)c->h_stage, W, rows, 0, BHRT_NFIELDS);
    return 0;
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
                        int S, int total, int root, devctx_t* rc, hipStream_t rs);

int bhrt_render_frame_gather(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                             const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                             IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                             int ndev_req, int shards_req, void* stream) {
    if (check_scene(bh, cfg) || !cam || !out || W <= 0 || H <= 0) {
        if (!g_err[0]) set_err("invalid argument");
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
    const int root = current_device();
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
    devctx_t* rc = ctx_get(root);
    if (!rc || (!stream && ctx_streams(rc))) return -1;
    hipStream_t rs = stream ? (hipStream_t)stream : rc->stream;
    /* NULL stream: the root's work -- the only writes into device_out -- is ordered like the
     * legacy default stream's (null_fence); the peers render into libbhrt's own buffers */
    const int fence = !stream && !null_unordered();
    if (fence && null_fence(rc, 0)) return -1;
    const int e = gather_frame(bh, dk, cfg, cam, W, H, method, flags, out, ndev, S, total, root,
                               rc, rs);
    if (fence && hipSetDevice(root) == hipSuccess && null_fence(rc, 1)) return -1;
    return e;
}

static int gather_frame(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                        const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                        IntegrationMethod method, int flags, const bhrt_frame_soa* out, int ndev,
                        int S, int total, int root, devctx_t* rc, hipStream_t rs) {
    const int B = 8;
    if (S == 1)
        return render_frame_device(bh, dk, cfg, cam, W, H, NULL, method, flags, out, rs, 0);
    const bhrt_frame_soa fields = device_fields(out, (int)method, dk != NULL, bh->spin != 0.0);
    bhrt_frame_soa shard_soa[BHRT_GATHER_MAX_SHARDS];
    int rc_all = 0;
    for (int k = 0; k < ndev && rc_all == 0; k++) { /* every device renders its shards */
        const int d = (root + k) % total;
        devctx_t* c = ctx_get(d);
        if (!c || hipSetDevice(d) != hipSuccess) {
            if (c) set_err("hipSetDevice(%d) failed", d);
            rc_all = -1;
            break;
        }
        if (k > 0 && ctx_streams(c)) {
            rc_all = -1;
            break;
        }
        hipStream_t st = k == 0 ? rs : c->stream;
        size_t bytes = 0;
        for (int s = k; s < S; s += ndev) {
            const bhrt_rows r = {B, s, S};
            bytes += soa_bytes(&fields, (long)bhrt_shard_rows(H, &r) * W);
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
        if (ensure(&c->d_gather, &c->cap_gather, need, 0) || lazy_event(&c->g_done) ||
            lazy_event(&c->g_copied)) {
            rc_all = -1;
            break;
        }
        char* p = (char*)c->d_gather;
        for (int s = k; s < S && rc_all == 0; s += ndev) {
            const bhrt_rows r = {B, s, S};
            soa_carve(&p, &fields, (long)bhrt_shard_rows(H, &r) * W, &shard_soa[s]);
            rc_all = render_frame_device(bh, dk, cfg, cam, W, H, &r, method, flags, &shard_soa[s],
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
        HIP_TRY(hipStreamWaitEvent(rs, g_ctx[(root + k) % total]->g_done, 0));
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
        devctx_t* c = g_ctx[(root + k) % total];
        c->g_wait = rc->g_copied;
        c->g_wait_pending = 1;
    }
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

/* drain every stream of the first ndev devices (keeps the current error text): a frame that
 * failed part way may still have launches and copies queued on its slot's buffers */
static void drain_devices(int ndev) {
    char err[sizeof g_err];
    memcpy(err, g_err, sizeof err);
    for (int d = 0; d < ndev; d++) {
        devctx_t* c = g_ctx[d];
        if (!c || hipSetDevice(d) != hipSuccess) continue;
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (c->stream2) (void)hipStreamSynchronize(c->stream2);
        for (int i = 0; i < 2; i++)
            if (c->xs[i]) (void)hipStreamSynchronize(c->xs[i]);
        if (c->copy) (void)hipStreamSynchronize(c->copy);
    }
    memcpy(g_err, err, sizeof err);
}

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
     * before the slot can be reused (ensure() may reallocate what a DMA still targets) */
    if (rc != 0) drain_devices(f->ndev);
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
    drain_devices(ndev);
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
    const bhrt_frame_soa fields = device_fields(host, (int)method, dk != NULL, bh->spin != 0.0);
    for (int d = 0; d < ndev; d++) { /* device buffers: every chunk of device d */
        devctx_t* c = ctx_get(d);
        if (!c) return -1;
        HIP_TRY(hipSetDevice(d));
        if (ctx_streams(c)) return -1;
        size_t dev_bytes = 0;
        for (int k = 0; k < K; k++) {
            bhrt_rows* r = &f->rows[k][d];
            r->row_block = block;
            r->shard = k * ndev + d;
            r->num_shards = shards;
            f->jobs[k][d].c = c;
            f->jobs[k][d].n = shards > 1 ? (long)bhrt_shard_rows(H, r) * W : (long)W * H;
            dev_bytes += soa_bytes(&fields, f->jobs[k][d].n);
        }
        if (ensure(&c->fr[slot].d_soa, &c->fr[slot].cap_soa, dev_bytes ? dev_bytes : 256, 0))
            return -1;
        char* p = (char*)c->fr[slot].d_soa;
        for (int k = 0; k < K; k++) soa_carve(&p, &fields, f->jobs[k][d].n, &f->jobs[k][d].dev);
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
                render_frame_device(bh, dk, cfg, cam, W, H, shards > 1 ? &f->rows[k][d] : NULL,
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
        if (ensure(&c->fr[slot].h_stage, &c->fr[slot].cap_stage, host_bytes ? host_bytes : 64, 1))
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
    if (check_scene(bh, cfg) || !cam || !host || W <= 0 || H <= 0) {
        if (!g_err[0]) set_err("invalid argument");
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
    if (check_scene(bh, cfg) || !rays || !host || n < 0) {
        if (!g_err[0]) set_err("invalid argument");
        return -1;
    }
    if (n == 0) return 0;
    int ndev = bhrt_device_count();
    if (ndev <= 0) {
        set_err("no HIP device available (libbhrt has no CPU path)");
        return -1;
    }
    if (n < 4096 * ndev) ndev = 1; /* small batches: one device, one launch */
    shard_job jobs[BHRT_MAX_DEV];
    long base[BHRT_MAX_DEV + 1];
    for (int d = 0; d <= ndev; d++) base[d] = (long)n * d / ndev;
    for (int d = 0; d < ndev; d++) {
        devctx_t* c = ctx_get(d);
        if (!c) return -1;
        HIP_TRY(hipSetDevice(d));
        if (ctx_streams(c)) return -1;
        long m = base[d + 1] - base[d];
        jobs[d].c = c;
        jobs[d].n = m;
        if (ensure(&c->d_rays, &c->cap_rays, (size_t)m * sizeof(Ray), 0)) return -1;
        if (device_soa(c, m, host, (int)method, dk != NULL, bh->spin != 0.0, &jobs[d].dev)) return -1;
        HIP_TRY(hipMemcpyAsync(c->d_rays, rays + base[d], (size_t)m * sizeof(Ray),
                               hipMemcpyHostToDevice, c->stream));
        const int shared = shared_origin(rays + base[d], m, host_threads());
        if (trace_rays_device((const Ray*)c->d_rays, NULL, (int)m, bh, dk, cfg, method, flags,
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
    const int stage_threads = host_threads();
    const int timing = getenv("BHRT_HOST_TIMING") != NULL;
    const int tl = env_int("BHRT_HOST_TIMING", 0) == 2; /* + each chunk's GPU timeline */
    /* timing events recorded (bit 0: before a chunk's upload, 1: after it, 2: after its trace,
     * 3: after its download, 4: at the call's start); BHRT_HOST_TIMING=2 records all */
    const int mk = tl ? 31 : env_int("BHRT_BATCH_MARKERS", 0);
    /* trace streams the chunks rotate over (BHRT_BATCH_STREAMS): 2 -- with 4, every chunk
     * queued at once, C2 camera rays ran 158 instead of 172 Mrays/s (profiles/r04) */
    int nst = env_int("BHRT_BATCH_STREAMS", 2);
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
        devctx_t* c = ctx_get(d);
        if (!c) return -1;
        HIP_TRY(hipSetDevice(d));
        if (ctx_streams(c)) return -1;
        for (int i = 0; i + 2 < nst; i++)
            if (!c->xs[i] && own_stream(&c->xs[i])) {
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
        if (ensure(&c->d_rays, &c->cap_rays, (size_t)m * sizeof(Ray), 0) ||
            ensure(&c->d_soa, &c->cap_soa, (size_t)m * HIT_BYTES + 4096 * K, 0) ||
            ensure(&c->h_rays, &c->cap_hrays, (size_t)m * sizeof(Ray), 1) ||
            ensure(&c->h_stage, &c->cap_stage, (size_t)m * HIT_BYTES, 1))
            return -1;
    }
    for (int k = 0; k < K; k++)
        for (int d = 0; d < ndev; d++) {
            devctx_t* c = ctx_get(d);
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
                int diff = !env_int("BHRT_SHARED_ORIGIN", 1);
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
                if (trace_rays_device(diff ? dr : NULL, diff ? NULL : (const double*)dr, (int)m,
                                      bh, dk, cfg, INTEGRATOR_RK4, 0, &jobs[k][d].dev, st,
                                      diff ? NULL : &o))
                    return -1;
            }
            HIP_TRY(hipEventRecord(c->chunk_done[k], st));
            if (mk & 4) HIP_TRY(hipEventRecord(c->tev[k][2], st));
            /* chunk k's download is issued after chunk k + 1's upload (late = 1): both copy
             * directions can share one in-order DMA queue, and a download queued there waits for
             * its chunk's trace -- an upload issued behind it waited too, so chunk k + 1 could
             * not start before chunk k had ended and the two trace streams ran one after the
             * other (the 140 vs 205 Mrays/s "fresh-process mode" of VERDICT r5, DESIGN.md
             * section 4). BHRT_BATCH_LATE_D2H=0: the round-5 order (A/B). */
            const int late = env_int("BHRT_BATCH_LATE_D2H", 1) != 0;
            if (!late || k > 0)
                if (batch_download(jobs, off, late ? k - 1 : k, d, mk)) return -1;
            if (late && k == K - 1 && batch_download(jobs, off, k, d, mk)) return -1;
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
    if (nthreads <= 0) nthreads = host_threads();
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
    if (!ray || check_scene(bh, cfg)) return RAY_ERROR;
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

RayTraceResult integrate_photon_path(const Vector4D* position, const Vector3D* direction,
                                     const BlackHoleParams* bh, const SimulationConfig* cfg,
                                     IntegrationMethod method, Vector3D* path, int max_positions,
                                     int* num_positions, RayTraceHit* hit) {
    if (!position || !direction || check_scene(bh, cfg)) return RAY_ERROR;
    int dev = current_device();
    devctx_t* c = ctx_get(dev);
    if (!c || ctx_streams(c)) return RAY_ERROR;
    const int record = path != NULL && num_positions != NULL &&
                       (max_positions > 0 || *num_positions < max_positions);
    const int num_in = (path && max_positions <= 0 && num_positions) ? *num_positions : 0;
    size_t path_bytes = record && max_positions > 0 ? (size_t)max_positions * sizeof(Vector3D) : 0;
    /* layout: [hit SoA: 2 ints + 8 doubles][num][path] */
    size_t need = 128 + 64 + path_bytes;
    if (ensure(&c->d_rays, &c->cap_rays, need, 0)) return RAY_ERROR;
    char* d = (char*)c->d_rays;
    bhrt_frame_soa s;
    memset(&s, 0, sizeof s);
    s.result = (int32_t*)d;
    s.steps = (int32_t*)(d + 8);
    s.hit_x = (double*)(d + 16);
    s.hit_y = s.hit_x + 1;
    s.hit_z = s.hit_x + 2;
    s.distance = s.hit_x + 3;
    s.time_dilation = s.hit_x + 4;
    s.sky_x = s.hit_x + 5;
    s.sky_y = s.hit_x + 6;
    s.sky_z = s.hit_x + 7;
    int* d_num = (int*)(d + 128);
    Vector3D* d_path = path_bytes ? (Vector3D*)(d + 192) : NULL;
    bhrt_kparams kp;
    fill_scene(&kp, bh, NULL, cfg, method, 0);
    kp.src = BHRT_SRC_RAYS;
    kp.n = 1;
    kp.out = s;
    double o4[4] = {position->t, position->x, position->y, position->z};
    double d3[3] = {direction->x, direction->y, direction->z};
    if (bhrt_launch_path(&kp, o4, d3, d_path, max_positions, d_num, num_in, c->stream) != 0) {
        set_err("path kernel launch failed");
        return RAY_ERROR;
    }
    char h[128 + 64];
    if (hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        set_err("path kernel failed: %s", hipGetErrorString(hipGetLastError()));
        return RAY_ERROR;
    }
    int num = *(int*)(h + 128);
    if (d_path && num > 0) {
        int cnt = num < max_positions ? num : max_positions;
        if (hipMemcpy(path, d_path, (size_t)cnt * sizeof(Vector3D), hipMemcpyDeviceToHost) !=
            hipSuccess) {
            set_err("path readback failed");
            return RAY_ERROR;
        }
    }
    if (path && num_positions && max_positions > 0) *num_positions = num;
    RayTraceResult res = (RayTraceResult)(*(int32_t*)h);
    if (hit) {
        const double* v = (const double*)(h + 16);
        hit->result = res;
        hit->steps = *(int32_t*)(h + 8);
        hit->hit_position.x = v[0];
        hit->hit_position.y = v[1];
        hit->hit_position.z = v[2];
        hit->distance = v[3];
        hit->time_dilation = v[4];
        if (res == RAY_MAX_DISTANCE) {
            hit->sky_direction.x = v[5];
            hit->sky_direction.y = v[6];
            hit->sky_direction.z = v[7];
        }
    }
    return res;
}

/* raytracer.c:868-932 */
static void jitter(int sample, int spp, JitterMethod jm, double strength, double* ox,
                   double* oy) {
    *ox = 0.5;
    *oy = 0.5;
    switch (jm) {
    case JITTER_REGULAR_GRID: {
        int g = (int)sqrt((double)spp);
        int x = sample % g, y = sample / g;
        *ox = (x + 0.5) / g;
        *oy = (y + 0.5) / g;
    } break;
    case JITTER_RANDOM:
        *ox = (double)rand() / RAND_MAX;
        *oy = (double)rand() / RAND_MAX;
        break;
    case JITTER_HALTON:
    case JITTER_BLUE_NOISE:
        *ox = halton_sequence(sample, 2);
        *oy = halton_sequence(sample, 3);
        break;
    default: break;
    }
    if (strength != 1.0) {
        *ox = 0.5 + (*ox - 0.5) * strength;
        *oy = 0.5 + (*oy - 0.5) * strength;
    }
}

/* raytracer.c:1044-1167: all samples of the pixel are traced in one GPU launch. Disk
 * samples take the frame colour contract's disk colour (the reference reads the never
 * written RayTraceHit.color there). */
RayTraceResult trace_pixel(int px, int py, int W, int H, const Vector3D* cam_pos,
                           const Vector3D* cam_dir, const Vector3D* cam_up, double fov,
                           const BlackHoleParams* bh, const AccretionDiskParams* dk,
                           const SimulationConfig* cfg, const SupersamplingParams* ss,
                           const AdaptiveSamplingParams* as, double color_out[3]) {
    color_out[0] = color_out[1] = color_out[2] = 0.0;
    int samples = ss ? ss->samples_per_pixel : 1;
    if (as && as->enable_adaptive) { /* :1076-1093, edge_factor fixed at 1.0 */
        samples = as->min_samples;
        samples += (int)((as->max_samples - as->min_samples) * 1.0);
        if (samples > as->max_samples) samples = as->max_samples;
    }
    RayTraceResult result = RAY_BACKGROUND;
    if (samples > 0) {
        if (!cam_pos || !cam_dir || !cam_up || check_scene(bh, cfg)) return RAY_ERROR;
        Ray* rays = (Ray*)malloc(sizeof(Ray) * (size_t)samples);
        double* rgb = (double*)malloc(sizeof(double) * 3 * (size_t)samples);
        int32_t* res = (int32_t*)malloc(sizeof(int32_t) * (size_t)samples);
        if (!rays || !rgb || !res) {
            free(rays); free(rgb); free(res);
            return RAY_ERROR;
        }
        bhrt_camera cam = {*cam_pos, *cam_dir, *cam_up, fov, 0, 0.0, 0.0};
        bhrt_kparams basis;
        fill_scene(&basis, bh, dk, cfg, INTEGRATOR_RK4, 0);
        fill_camera(&basis, &cam, W, H);
        for (int s = 0; s < samples; s++) {
            double ox = 0.5, oy = 0.5;
            if (ss && ss->samples_per_pixel > 1)
                jitter(s, ss->samples_per_pixel, ss->jitter_method, ss->jitter_strength, &ox, &oy);
            double ndcx = (2.0 * ((px + ox) / W) - 1.0) * basis.cam.plane_w;
            double ndcy = (1.0 - 2.0 * ((py + oy) / H)) * basis.cam.plane_h;
            Vector3D f = {basis.cam.fwd[0], basis.cam.fwd[1], basis.cam.fwd[2]};
            Vector3D r = {basis.cam.right[0], basis.cam.right[1], basis.cam.right[2]};
            Vector3D u = {basis.cam.up[0], basis.cam.up[1], basis.cam.up[2]};
            Vector3D d = vector3D_add(f, vector3D_scale(r, ndcx));
            d = vector3D_add(d, vector3D_scale(u, ndcy));
            rays[s].origin = *cam_pos;
            rays[s].direction = vector3D_normalize(d);
        }
        bhrt_frame_soa soa;
        memset(&soa, 0, sizeof soa);
        soa.result = res;
        soa.rgb_r = rgb;
        soa.rgb_g = rgb + samples;
        soa.rgb_b = rgb + 2 * samples;
        int rc = bhrt_trace_rays(rays, samples, bh, dk, cfg, INTEGRATOR_RK4, 0, &soa);
        if (rc == 0) {
            result = (RayTraceResult)res[0];
            for (int s = 0; s < samples; s++) {
                color_out[0] += soa.rgb_r[s];
                color_out[1] += soa.rgb_g[s];
                color_out[2] += soa.rgb_b[s];
            }
        }
        free(rays); free(rgb); free(res);
        if (rc != 0) return RAY_ERROR;
    }
    color_out[0] /= samples;
    color_out[1] /= samples;
    color_out[2] /= samples;
    return result;
}

/* ======================================================================================= */
/* what supersample.c and paths.c build on (bhrt_host.h): wrappers only                     */
/* ======================================================================================= */
void* bhrt_hook_ctx(void) { return ctx_get(current_device()); }

void* bhrt_hook_ctx_stream(void* ctx) {
    devctx_t* c = (devctx_t*)ctx;
    return ctx_streams(c) == 0 ? (void*)c->stream : NULL;
}

void* bhrt_hook_scratch(void* ctx, void* stream, size_t bytes) {
    return stream_scratch((devctx_t*)ctx, (hipStream_t)stream, bytes);
}

void* bhrt_hook_ss_buffer(void* ctx, size_t bytes) {
    devctx_t* c = (devctx_t*)ctx;
    return ensure(&c->d_ss, &c->cap_ss, bytes ? bytes : 256, 0) ? NULL : c->d_ss;
}

int bhrt_hook_null_unordered(void) { return null_unordered(); }

int bhrt_hook_null_fence(void* ctx, int after) { return null_fence((devctx_t*)ctx, after); }

int bhrt_hook_trace_dirs(const double* d_dirs, int n, const BlackHoleParams* bh,
                         const AccretionDiskParams* dk, const SimulationConfig* cfg,
                         IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                         void* stream, const Vector3D* origin) {
    return trace_rays_device(NULL, d_dirs, n, bh, dk, cfg, method, flags, out, stream, origin);
}

int bhrt_hook_trace_rays(const Ray* d_rays, int n, const BlackHoleParams* bh,
                         const AccretionDiskParams* dk, const SimulationConfig* cfg,
                         IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                         void* stream) {
    return trace_rays_device(d_rays, NULL, n, bh, dk, cfg, method, flags, out, stream, NULL);
}

void bhrt_hook_fill_camera(bhrt_kparams* kp, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg,
                           IntegrationMethod method, int flags, const bhrt_camera* cam, int W,
                           int H) {
    fill_scene(kp, bh, dk, cfg, method, flags);
    fill_camera(kp, cam, W, H);
}

int bhrt_hook_scene(bhrt_kparams* kp, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                    const SimulationConfig* cfg, IntegrationMethod method, int flags) {
    if (check_scene(bh, cfg)) return -1;
    return fill_scene(kp, bh, dk, cfg, method, flags);
}

int bhrt_hook_launch(void* ctx, bhrt_kparams* kp, void* stream, bhrt_launch_fn fn,
                     const void* arg) {
    return launch_fn((devctx_t*)ctx, kp, (hipStream_t)stream, fn, arg);
}

int bhrt_hook_colour_fused(int method, int has_disk, int spin) {
    return colour_fused(method, has_disk, spin);
}

void bhrt_hook_jitter(int sample, int spp, JitterMethod jm, double strength, double* ox,
                      double* oy) {
    jitter(sample, spp, jm, strength, ox, oy);
}

/* ======================================================================================= */
/* scalar helpers of the ray path (host side of the drop-in)                                */
/* ======================================================================================= */
int check_disk_intersection(const Vector3D* p, const Vector3D* v, const Vector3D* n,
                            const AccretionDiskParams* disk, Vector3D* q) {
    double den = vector3D_dot(*v, *n);
    if (fabs(den) < BH_EPSILON) return 0;
    double t = -(vector3D_dot(*p, *n)) / den;
    if (t < 0.0) return 0;
    *q = vector3D_add(*p, vector3D_scale(*v, t));
    double r = sqrt(q->x * q->x + q->y * q->y);
    return r >= disk->inner_radius && r <= disk->outer_radius;
}

void temperature_to_rgb(double T, double rgb[3]) {
    T = clamp(T, 1000.0, 40000.0);
    double t = (T - 1000.0) / (40000.0 - 1000.0);
    rgb[0] = t < 0.5 ? t * 2.0 : 1.0;
    rgb[1] = t < 0.25 ? 0.0 : (t < 0.75 ? (t - 0.25) * 2.0 : 1.0);
    rgb[2] = t < 0.5 ? 0.0 : (t - 0.5) * 2.0;
    double br = 0.2 + 0.8 * (t * t);
    rgb[0] *= br;
    rgb[1] *= br;
    rgb[2] *= br;
}

void calculate_disk_temperature(const Vector3D* p, const BlackHoleParams* bh,
                                const AccretionDiskParams* disk, double* T, double color[3]) {
    (void)bh;
    double r = sqrt(p->x * p->x + p->y * p->y);
    double nr = clamp((r - disk->inner_radius) / (disk->outer_radius - disk->inner_radius), 0.0, 1.0);
    *T = disk->temperature_scale * (2000.0 + 18000.0 * pow(1.0 - nr, 0.75));
    temperature_to_rgb(*T, color);
}

double calculate_time_dilation(double r, const BlackHoleParams* bh) {
    return 1.0 / sqrt(1.0 - bh->schwarzschild_radius / r);
}

void apply_relativistic_effects(const Vector3D* p, const Vector3D* v, const BlackHoleParams* bh,
                                double c[3], double* dop_out) {
    double r = sqrt(p->x * p->x + p->y * p->y);
    double phi = atan2(p->y, p->x);
    Vector3D tangent = {-sin(phi), cos(phi), 0.0};
    double dop = 1.0 + vector3D_dot(*v, tangent) * 0.5;
    double z = dop / calculate_time_dilation(r, bh);
    if (z < 1.0) {
        c[2] *= z;
        c[0] = fmin(1.0, c[0] * (2.0 - z));
    } else {
        c[0] *= 2.0 - z;
        c[2] = fmin(1.0, c[2] * z);
    }
    double beam = pow(dop, 4);
    c[0] = clamp(c[0] * beam, 0.0, 1.0);
    c[1] = clamp(c[1] * beam, 0.0, 1.0);
    c[2] = clamp(c[2] * beam, 0.0, 1.0);
    if (dop_out) *dop_out = dop;
}

void generate_gpu_shader_params(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                                double observer_distance, double fov, GPUShaderParams* p) {
    if (!bh || !p) return;
    p->mass = bh->mass;
    p->spin = bh->spin;
    p->schwarzschild_radius = 2.0 * bh->mass;
    p->observer_distance = observer_distance;
    p->fov = fov;
    if (dk) {
        p->disk_inner_radius = dk->inner_radius;
        p->disk_outer_radius = dk->outer_radius;
        p->disk_temp_scale = dk->temperature_scale;
    } else {
        p->disk_inner_radius = 3.0 * p->schwarzschild_radius;
        p->disk_outer_radius = 20.0 * p->schwarzschild_radius;
        p->disk_temp_scale = 1.0;
    }
}

double halton_sequence(int index, int base) {
    double result = 0.0, f = 1.0;
    for (; index > 0; index /= base) {
        f /= base;
        result += f * (index % base);
    }
    return result;
}

SchwarzschildMetric calculate_schwarzschild_metric(double r, const BlackHoleParams* bh) {
    SchwarzschildMetric m;
    double rs = bh->schwarzschild_radius;
    if (r <= rs + BH_EPSILON) r = rs + BH_EPSILON;
    m.g_tt = -(1.0 - rs / r);
    m.g_rr = 1.0 / (1.0 - rs / r);
    m.g_thth = r * r;
    m.g_phph = r * r; /* r*r*sin^2(pi/2), sin(pi/2) == 1.0 in double */
    return m;
}

void cartesian_to_spherical(const Vector3D* c, Vector3D* s) {
    double r = sqrt(c->x * c->x + c->y * c->y + c->z * c->z);
    double th = r > BH_EPSILON ? acos(c->z / r) : 0.0;
    double ph = atan2(c->y, c->x);
    if (ph < 0.0) ph += BH_TWO_PI;
    s->x = r;
    s->y = th;
    s->z = ph;
}

void spherical_to_cartesian(const Vector3D* s, Vector3D* c) {
    c->x = s->x * sin(s->y) * cos(s->z);
    c->y = s->x * sin(s->y) * sin(s->z);
    c->z = s->x * cos(s->y);
}

double get_isco_radius(const BlackHoleParams* bh) {
    double M = bh->mass, a = bh->spin * M;
    if (bh->spin == 0.0) return 6.0 * M;
    double third = 1.0 / 3.0;
    double z1 = 1.0 + pow(1.0 - a * a / (M * M), third) *
                          (pow(1.0 + a / (M), third) + pow(1.0 - a / (M), third));
    double z2 = sqrt(3.0 * a * a / (M * M) + z1 * z1);
    return M * (3.0 + z2 - sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2)));
}

void initialize_black_hole_params(BlackHoleParams* bh, double mass, double spin, double charge) {
    bh->mass = mass;
    bh->spin = spin;
    bh->charge = charge;
    bh->schwarzschild_radius = 2.0 * mass; /* every branch: spacetime.c:338,348,358 */
    bh->ergosphere_radius = 2.0 * mass;
    if (spin == 0.0 && charge == 0.0) {
        bh->r_plus = 2.0 * mass;
        bh->r_minus = 0.0;
    } else {
        double a = spin * mass;
        double q2 = (spin > 0.0 && charge == 0.0) ? 0.0 : charge * charge;
        double s = q2 == 0.0 ? sqrt(mass * mass - a * a) : sqrt(mass * mass - a * a - q2);
        bh->r_plus = mass + s;
        bh->r_minus = mass - s;
    }
    bh->isco_radius = get_isco_radius(bh);
}

/* ---- generic host integrators (math_util.c:162-457; debug printing not reproduced) ---- */
void rk4_integrate(ODEFunction f, double* y, int n, double t, double h, void* params) {
    double* w = (double*)malloc(sizeof(double) * 5 * (size_t)(n > 0 ? n : 1));
    if (!w) return;
    double *k1 = w, *k2 = w + n, *k3 = w + 2 * n, *k4 = w + 3 * n, *yt = w + 4 * n;
    f(t, y, k1, params);
    for (int i = 0; i < n; i++) yt[i] = y[i] + 0.5 * h * k1[i];
    f(t + 0.5 * h, yt, k2, params);
    for (int i = 0; i < n; i++) yt[i] = y[i] + 0.5 * h * k2[i];
    f(t + 0.5 * h, yt, k3, params);
    for (int i = 0; i < n; i++) yt[i] = y[i] + h * k3[i];
    f(t + h, yt, k4, params);
    for (int i = 0; i < n; i++) y[i] += h * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) / 6.0;
    free(w);
}

int rkf45_integrate(ODEFunction f, double y[], int n, double* t, double h, double* h_next,
                    double eps_rel, void* params) {
    static const double A[6] = {0.0, 1.0 / 4.0, 3.0 / 8.0, 12.0 / 13.0, 1.0, 1.0 / 2.0};
    static const double B[6][5] = {
        {0, 0, 0, 0, 0},
        {1.0 / 4.0, 0, 0, 0, 0},
        {3.0 / 32.0, 9.0 / 32.0, 0, 0, 0},
        {1932.0 / 2197.0, -7200.0 / 2197.0, 7296.0 / 2197.0, 0, 0},
        {439.0 / 216.0, -8.0, 3680.0 / 513.0, -845.0 / 4104.0, 0},
        {-8.0 / 27.0, 2.0, -3544.0 / 2565.0, 1859.0 / 4104.0, -11.0 / 40.0}};
    static const double C4[6] = {25.0 / 216.0, 0, 1408.0 / 2565.0, 2197.0 / 4104.0, -1.0 / 5.0, 0};
    static const double C5[6] = {16.0 / 135.0, 0, 6656.0 / 12825.0, 28561.0 / 56430.0,
                                 -9.0 / 50.0, 2.0 / 55.0};
    double* w = (double*)malloc(sizeof(double) * 9 * (size_t)(n > 0 ? n : 1));
    if (!w) return 1;
    double* k[6];
    for (int s = 0; s < 6; s++) k[s] = w + s * n;
    double *yt = w + 6 * n, *y4 = w + 7 * n, *y5 = w + 8 * n;
    int rc = 1;
    f(*t, y, k[0], params);
    for (int i = 0; i < n; i++)
        if (isnan(k[0][i]) || isinf(k[0][i])) goto out;
    for (int s = 1; s < 6; s++) {
        for (int i = 0; i < n; i++) {
            /* same left-to-right sums as the unrolled reference: h*b21*k1 for stage 2,
             * h*(b31*k1 + b32*k2 + ...) afterwards */
            double acc;
            if (s == 1) {
                yt[i] = y[i] + h * B[1][0] * k[0][i];
                continue;
            }
            acc = B[s][0] * k[0][i];
            for (int j = 1; j < s; j++) acc = acc + B[s][j] * k[j][i];
            yt[i] = y[i] + h * acc;
        }
        f(*t + h * A[s], yt, k[s], params);
    }
    double max_error = 0.0;
    for (int i = 0; i < n; i++) {
        y4[i] = y[i] + h * (C4[0] * k[0][i] + C4[2] * k[2][i] + C4[3] * k[3][i] + C4[4] * k[4][i]);
        y5[i] = y[i] + h * (C5[0] * k[0][i] + C5[2] * k[2][i] + C5[3] * k[3][i] +
                            C5[4] * k[4][i] + C5[5] * k[5][i]);
        double scale = fmax(fabs(y[i]), fabs(y5[i]));
        if (scale < BH_EPSILON) scale = BH_EPSILON;
        max_error = fmax(max_error, fabs(y5[i] - y4[i]) / scale);
    }
    double ratio = max_error / eps_rel;
    if (ratio <= 1.0) {
        double scale = ratio == 0.0 ? 10.0 : fmax(0.2, fmin(10.0, 0.9 * pow(ratio, -0.2)));
        for (int i = 0; i < n; i++) y[i] = y5[i];
        *t = *t + h;
        *h_next = h * scale;
        rc = 0;
    } else {
        *h_next = h * fmax(0.2, fmin(10.0, 0.9 * pow(ratio, -0.25)));
    }
out:
    free(w);
    return rc;
}

/* ======================================================================================= */
/* context API (src/blackhole_api.c)                                                       */
/* ======================================================================================= */
BHContextHandle bh_initialize(void) { /* blackhole_api.c:52-80 */
    BHContextHandle c = (BHContextHandle)calloc(1, sizeof(struct BHContext_t));
    if (!c) return NULL;
    c->blackhole.mass = 1.0;
    c->blackhole.schwarzschild_radius = 2.0;
    c->disk.inner_radius = 6.0;
    c->disk.outer_radius = 20.0;
    c->disk.temperature_scale = 1.0;
    c->disk.density_scale = 1.0;
    c->config.time_step = 0.1;
    c->config.max_ray_distance = 100.0;
    c->config.max_integration_steps = 1000;
    c->config.tolerance = 1.0e-6;
    return c;
}

void bh_shutdown(BHContextHandle c) { free(c); }

double blackhole_get_mass(BHContextHandle c) { return c ? c->blackhole.mass : 0.0; }

void bh_calculate_orbital_velocity(BHContextHandle c, double r, double* v_phi) {
    if (!c || !v_phi || r <= 0) return;
    *v_phi = sqrt(blackhole_get_mass(c) / r);
}

BHErrorCode bh_configure_black_hole(BHContextHandle c, double mass, double spin, double charge) {
    if (!c || mass <= 0.0 || spin < 0.0 || spin > 1.0) return BH_ERROR_INVALID_PARAMETER;
    initialize_black_hole_params(&c->blackhole, mass, spin, charge);
    return BH_SUCCESS;
}

BHErrorCode bh_configure_accretion_disk(BHContextHandle c, double inner, double outer,
                                        double tscale, double density) {
    if (!c || inner <= 0.0 || outer <= inner || tscale <= 0.0 || density <= 0.0)
        return BH_ERROR_INVALID_PARAMETER;
    c->disk.inner_radius = inner;
    c->disk.outer_radius = outer;
    c->disk.temperature_scale = tscale;
    c->disk.density_scale = density;
    c->disk_enabled = 1;
    return BH_SUCCESS;
}

BHErrorCode bh_configure_simulation(BHContextHandle c, double dt, double max_dist, int max_steps,
                                    double tol) {
    if (!c || dt <= 0.0 || max_dist <= 0.0 || max_steps <= 0 || tol <= 0.0)
        return BH_ERROR_INVALID_PARAMETER;
    c->config.time_step = dt;
    c->config.max_ray_distance = max_dist;
    c->config.max_integration_steps = max_steps;
    c->config.tolerance = tol;
    return BH_SUCCESS;
}

BHErrorCode bh_trace_ray(BHContextHandle c, const double origin[3], const double direction[3],
                         RayTraceHit* hit) {
    if (!c || !origin || !direction || !hit) return BH_ERROR_INVALID_PARAMETER;
    Ray ray;
    ray.origin.x = origin[0];
    ray.origin.y = origin[1];
    ray.origin.z = origin[2];
    Vector3D d = {direction[0], direction[1], direction[2]};
    ray.direction = vector3D_normalize(d); /* blackhole_api.c:203-204 */
    RayTraceResult r = trace_ray(&ray, &c->blackhole, c->disk_enabled ? &c->disk : NULL,
                                 &c->config, hit);
    return r == RAY_ERROR ? BH_ERROR_SIMULATION : BH_SUCCESS;
}

BHErrorCode bh_trace_rays_batch(BHContextHandle c, const Ray* rays, RayTraceHit* hits, int count) {
    if (!c || !rays || !hits || count <= 0) return BH_ERROR_INVALID_PARAMETER;
    if (trace_rays_batch(rays, count, &c->blackhole, c->disk_enabled ? &c->disk : NULL,
                         &c->config, hits, 0) != 0)
        return BH_ERROR_SIMULATION;
    for (int i = 0; i < count; i++)
        if (hits[i].result == RAY_ERROR) return BH_ERROR_SIMULATION;
    return BH_SUCCESS;
}

BHErrorCode bh_calculate_time_dilation(BHContextHandle c, const double p1[3], const double p2[3],
                                       double* ratio) {
    if (!c || !p1 || !p2 || !ratio) return BH_ERROR_INVALID_PARAMETER;
    double r1 = sqrt(p1[0] * p1[0] + p1[1] * p1[1] + p1[2] * p1[2]);
    double r2 = sqrt(p2[0] * p2[0] + p2[1] * p2[1] + p2[2] * p2[2]);
    *ratio = calculate_time_dilation(r1, &c->blackhole) / calculate_time_dilation(r2, &c->blackhole);
    return BH_SUCCESS;
}

void bh_get_version(int* major, int* minor, int* patch) {
    if (major) *major = BLACKHOLE_API_VERSION_MAJOR;
    if (minor) *minor = BLACKHOLE_API_VERSION_MINOR;
    if (patch) *patch = BLACKHOLE_API_VERSION_PATCH;
}

/* blackhole_api.c:495-608: packs a float parameter block for a shader */
BHErrorCode bh_generate_shader_data(void* context, const float pos[3], const float dir[3],
                                    const float up[3], int width, int height, float fov,
                                    int enable_doppler, int enable_redshift, int show_disk,
                                    float* out) {
    if (!context || !pos || !dir || !up || !out) return BH_ERROR_INVALID_PARAMETER;
    BHContextHandle c = (BHContextHandle)context;
    struct {
        float mass, spin, schwarzschild_radius, r_isco, r_horizon;
        float disk_inner_radius, disk_outer_radius, disk_temp_scale, disk_density_scale;
        float observer_pos[3], observer_dir[3], up_vector[3];
        float fov, aspect_ratio;
        int enable_doppler, enable_redshift, show_disk;
        int max_steps;
        float step_size, tolerance, max_distance;
        float padding[4];
    } p;
    p.mass = (float)c->blackhole.mass;
    p.spin = (float)c->blackhole.spin;
    p.schwarzschild_radius = (float)c->blackhole.schwarzschild_radius;
    p.r_isco = (float)c->blackhole.isco_radius;
    p.r_horizon = (float)c->blackhole.r_plus;
    int disk_on = show_disk && c->disk_enabled;
    p.disk_inner_radius = disk_on ? (float)c->disk.inner_radius : 1000.0f;
    p.disk_outer_radius = disk_on ? (float)c->disk.outer_radius : 100.0f;
    p.disk_temp_scale = disk_on ? (float)c->disk.temperature_scale : 0.0f;
    p.disk_density_scale = disk_on ? (float)c->disk.density_scale : 0.0f;
    memcpy(p.observer_pos, pos, sizeof p.observer_pos);
    memcpy(p.observer_dir, dir, sizeof p.observer_dir);
    memcpy(p.up_vector, up, sizeof p.up_vector);
    p.fov = fov * (float)BH_PI / 180.0f;
    p.aspect_ratio = (float)width / (float)height;
    p.enable_doppler = enable_doppler;
    p.enable_redshift = enable_redshift;
    p.show_disk = disk_on;
    p.max_steps = c->config.max_integration_steps;
    p.step_size = (float)c->config.time_step;
    p.tolerance = (float)c->config.tolerance;
    p.max_distance = (float)c->config.max_ray_distance;
    memset(p.padding, 0, sizeof p.padding);
    memcpy(out, &p, sizeof p);
    return BH_SUCCESS;
}
