/*
 * context.c -- the per-thread state of libbhrt's host layer: the error text, and per (host
 * thread, device) a context with its streams, growable buffers and a ring of control blocks
 * (queue heads + counters) with start/stop events per launch, so the entry points stay callable
 * concurrently from several host threads (SURVEY.md 8b "Threading"). Every kernel launch that is
 * timed and counted goes through bhrt_ctx_launch_fn; bhrt_get_stats reads the counters back.
 *
 * There is no CPU fallback: a HIP failure is reported through the reference's error value
 * (RAY_ERROR / -1 / BH_ERROR_SIMULATION) and bhrt_last_error().
 */
#define _GNU_SOURCE
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"

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

const char* bhrt_last_error(void) { return g_err; }
int bhrt_err_is_set(void) { return g_err[0] != 0; }

/* ======================================================================================= */
/* device contexts                                                                          */
/* ======================================================================================= */
static _Thread_local devctx_t* g_ctx[BHRT_MAX_DEV];
static _Thread_local bhrt_stats g_stats;

int bhrt_env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

int bhrt_current_device(void) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return -1;
    return d;
}

int bhrt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    const char* cap = getenv("BHRT_MAX_DEVICES");
    if (cap && atoi(cap) > 0 && atoi(cap) < n) n = atoi(cap);
    if (n > BHRT_MAX_DEV) n = BHRT_MAX_DEV;
    return n;
}

devctx_t* bhrt_ctx_get(int device) {
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
int bhrt_own_stream(hipStream_t* s) {
    const int mode = bhrt_env_int("BHRT_STREAM_QUEUE", 1);
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

int bhrt_ctx_streams(devctx_t* c) {
    if (c->stream && c->stream2 && c->copy) return 0;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != c->device) {
        if (hipSetDevice(c->device) != hipSuccess) {
            set_err("hipSetDevice(%d) failed", c->device);
            return -1;
        }
    }
    if ((!c->stream && bhrt_own_stream(&c->stream)) || (!c->stream2 && bhrt_own_stream(&c->stream2)) ||
        (!c->copy && bhrt_own_stream(&c->copy))) {
        set_err("cannot create libbhrt's streams on device %d", c->device);
        if (cur >= 0 && cur != c->device) (void)hipSetDevice(cur);
        return -1;
    }
    if (cur >= 0 && cur != c->device && hipSetDevice(cur) != hipSuccess) return -1;
    return 0;
}

int bhrt_ensure(void** p, size_t* cap, size_t need, int pinned) {
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

/* one of the context's per-stream blocks of `stream`, at least `bytes` */
static void* stream_block(bhrt_stream_block* tab, int* next, hipStream_t stream, size_t bytes) {
    int slot = -1;
    for (int i = 0; i < BHRT_SCRATCH_SLOTS; i++)
        if (tab[i].p && tab[i].stream == stream) slot = i;
    if (slot < 0) {
        slot = *next;
        *next = (*next + 1) % BHRT_SCRATCH_SLOTS;
        if (tab[slot].p && hipStreamSynchronize(tab[slot].stream) != hipSuccess) {
            set_err("hipStreamSynchronize failed");
            return NULL;
        }
        tab[slot].stream = stream;
    } else if (tab[slot].cap < bytes &&
               hipStreamSynchronize(stream) != hipSuccess) { /* in use until drained */
        set_err("hipStreamSynchronize failed");
        return NULL;
    }
    if (bhrt_ensure(&tab[slot].p, &tab[slot].cap, bytes ? bytes : 64, 0)) return NULL;
    return tab[slot].p;
}

/* launch scratch of `stream` on this context, at least `bytes` */
void* bhrt_stream_scratch(devctx_t* c, hipStream_t stream, size_t bytes) {
    return stream_block(c->scratch, &c->scratch_next, stream, bytes);
}

/* the second block of `stream`: never moved or freed by a request for the first */
void* bhrt_stream_keep(devctx_t* c, hipStream_t stream, size_t bytes) {
    return stream_block(c->keep, &c->keep_next, stream, bytes);
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

/* drain every stream of the first ndev devices (keeps the current error text): a frame that
 * failed part way may still have launches and copies queued on its slot's buffers */
void bhrt_drain_devices(int ndev) {
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

/* ======================================================================================= */
/* launch plumbing                                                                          */
/* ======================================================================================= */
/* one timed kernel launch on `stream` (the context's own if NULL) with a control block of the
 * ring: the trace kernel (fn NULL), or fn(kp, arg, stream, ev0, ev1) -- a launcher with
 * bhrt_launch_trace's contract that another host file names */
int bhrt_ctx_launch_fn(devctx_t* c, bhrt_kparams* kp, hipStream_t stream, bhrt_launch_fn fn,
                       const void* arg) {
    if (kp->n <= 0) return 0;
    if (!stream) {
        if (bhrt_ctx_streams(c)) return -1;
        stream = c->stream;
    }
    /* the redo list follows the initial-state table (one extra field of the allocation) */
    if (kp->init) kp->redo = (int*)(kp->init + (size_t)BHRT_INIT_FIELDS * (size_t)kp->n);
    /* a sky frame's separate colour pass reads the exit chords from the three fields behind it */
    if (kp->sky.tex && !fn) {
        if (bhrt_sky_check(kp->sc.flags, c->device)) return -1;
        kp->sky.chord = kp->init && !kp->colour_fused
                            ? kp->init + (size_t)(BHRT_INIT_FIELDS + 1) * (size_t)kp->n
                            : NULL;
    }
    if (c->npend == BHRT_RING && harvest(c, 1, stream, BHRT_RING / 2) != 0) return -1;
    if (ring_order(c, stream)) return -1;
    int slot = c->next_slot;
    c->next_slot = (c->next_slot + 1) % BHRT_RING;
    kp->ctl = c->d_ctl + (size_t)slot * BHRT_SLOT_WORDS;
    kp->qhead = kp->ctl + BHRT_QHEAD_OFF;
    kp->diag_slot = slot;
    /* (the slot was zeroed when it was last harvested, or at the context's creation) */
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

/* A NULL hip_stream in the device API means what it means for a HIP launch: ordered after
 * every piece of work the caller queued on the legacy default stream (a hipMemset or a torch
 * fill of the outputs) and before everything queued there afterwards -- while the kernels
 * still run on libbhrt's own high-priority stream (bhrt_own_stream: its own hardware queue). Two
 * event hops per call, no host sync: the default stream -> libbhrt's stream before the launch
 * (bhrt_null_fence(c, 0)) and back after it (bhrt_null_fence(c, 1)). Round 5 launched NULL calls on
 * libbhrt's non-blocking stream with no ordering at all, and a torch fill still queued behind
 * the trace kernel overwrote 3.37 M of 4.15 M rays of a frame;
 * BHRT_NULL_STREAM=unordered keeps that behaviour as an explicit opt-in. */
int bhrt_null_unordered(void) {
    const char* e = getenv("BHRT_NULL_STREAM");
    return e && strcmp(e, "unordered") == 0;
}

int bhrt_null_fence(devctx_t* c, int after) {
    if (after) {
        HIP_TRY(hipEventRecord(c->nul_out, c->stream));
        HIP_TRY(hipStreamWaitEvent((hipStream_t)0, c->nul_out, 0));
    } else {
        HIP_TRY(hipEventRecord(c->nul_in, (hipStream_t)0));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->nul_in, 0));
    }
    return 0;
}

/* One launch body under that rule. A caller stream is used as given. A NULL stream runs the
 * body on the context's own stream between the two fences: -1 if either fails, else the body's
 * code. BHRT_NULL_STREAM=unordered leaves the fences out; the body then gets the context's own
 * stream -- or, from a caller that passes no context (bhrt_api.c's entry points, which make
 * theirs after their argument checks), the NULL itself, and the context is made here only for
 * the fences. */
int bhrt_on_stream(devctx_t* c, hipStream_t stream, bhrt_stream_body body, const void* arg) {
    if (stream) return body(c, stream, arg);
    if (!c) {
        if (bhrt_null_unordered()) return body(NULL, NULL, arg);
        c = bhrt_ctx_get(bhrt_current_device());
        if (!c || bhrt_ctx_streams(c)) return -1;
    } else {
        if (bhrt_ctx_streams(c)) return -1;
        if (bhrt_null_unordered()) return body(c, c->stream, arg);
    }
    if (bhrt_null_fence(c, 0)) return -1;
    const int rc = body(c, c->stream, arg);
    return bhrt_null_fence(c, 1) ? -1 : rc;
}
