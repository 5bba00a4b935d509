/*
 * bhrt_host.h -- the internal interface of libbhrt.so's C host files. Not installed; everything
 * declared here has hidden visibility. Prototypes are grouped by the module that owns them:
 *   ref_host.c     the reference's vector and scalar functions on the host (no HIP)
 *   context.c      per-thread errors, device contexts, streams, the control ring, launches
 *   scene.c        scene and origin set-up: the host arithmetic that decides a frame's bits
 *   bhrt_api.c     device frames and ray arrays, the SoA helpers, the multi-device gather
 *   host_frames.c  host-buffer frames in flight, readback, bhrt_trace_rays
 *   batch.c        trace_ray / trace_rays_batch: the pipelined chunks
 *   dropin.c       integrate_photon_path, trace_pixel, the bh_* context API
 *   supersample.c, adaptive.c, temporal.c, paths.c, particles.c, particles_resident.c, sky.c,
 *   kerr.c, kerr_paths.c, kerr_rk45.c, kerr_emit.c, kerr_particles.c
 *                  features with launchers of their own
 */
#ifndef BHRT_HOST_H
#define BHRT_HOST_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>

#pragma GCC visibility push(default)
#include "../../include/bhrt_api.h"
#pragma GCC visibility pop
#include "bhrt_kernel.h"

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
/* a launch's control block and its ray-queue heads are one region of the ring: 128 B of
 * counters, padding to 256 B, then the queue heads. The whole ring is zeroed by one fill on the
 * GPU after each harvest (context.c ring_order), never per launch. */
#define BHRT_QHEAD_OFF 32 /* u64 words */
#define BHRT_SLOT_WORDS (BHRT_QHEAD_OFF + BHRT_QWORDS)
#define BHRT_RING_BYTES ((size_t)BHRT_RING * BHRT_SLOT_WORDS * sizeof(unsigned long long))
#define BHRT_RING_STREAMS 8 /* streams remembered as ordered after the ring's last fill */
#define BHRT_MAX_CHUNKS 8   /* host-buffer frames: pipelined chunks per device            */
#define BHRT_SCRATCH_SLOTS 8
#define BHRT_FRAME_SLOTS 3  /* host-buffer frames in flight per thread (bhrt_render_frame_async) */
#define BHRT_COPY_PARTS 4   /* host-buffer frames: a chunk's D2H in parts, each un-permuted as it lands */

typedef struct { /* a growable device block bound to a stream */
    hipStream_t stream;
    void* p;
    size_t cap;
} bhrt_stream_block;

typedef struct {
    int slot;
    int redo; /* the redo pass was launched after the hot one */
    int untested; /* RKF45 attempts without the accept test (bhrt_scene_k.accept_all) */
    hipEvent_t ev0, ev1;
} pending_t;

/* the calling thread's state of one device */
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
    /* NULL hip_stream of the device API (bhrt_null_fence): the caller's default stream ->
     * libbhrt's stream before the launch, and back after it */
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
    bhrt_stream_block scratch[BHRT_SCRATCH_SLOTS];
    int scratch_next;
    /* a second block per stream (bhrt_stream_keep) for what must outlive a later, larger request
     * for the launch scratch: an adaptive frame's base planes across its second launch */
    bhrt_stream_block keep[BHRT_SCRATCH_SLOTS];
    int keep_next;
    /* adaptive.c: pinned staging of the edge count read back and the row tables uploaded */
    void* h_ad;
    size_t cap_ad;
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
    /* bhrt_render_frame_ss (supersample.c), bhrt_trace_paths (paths.c), the Kerr host forms
     * (kerr.c, kerr_paths.c): the device arrays of a call that returns only once its host arrays
     * are complete */
    void* d_ss;
    size_t cap_ss;
} devctx_t;

/* ---- context.c ---- */
/* per-thread error message read back by bhrt_last_error(); whether one is set */
void bhrt_set_err(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int bhrt_err_is_set(void);
#define set_err bhrt_set_err
#define HIP_TRY(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_err("%s failed: %s", #call, hipGetErrorString(e_));                           \
            return -1;                                                                        \
        }                                                                                     \
    } while (0)
int bhrt_env_int(const char* name, int dflt);
int bhrt_current_device(void); /* -1: none */
/* the calling thread's context of `device`, created on first use; NULL with the error set */
devctx_t* bhrt_ctx_get(int device);
/* libbhrt's own streams of a context (stream, stream2, copy), created on first use */
int bhrt_ctx_streams(devctx_t* c);
int bhrt_own_stream(hipStream_t* s);
int bhrt_ensure(void** p, size_t* cap, size_t need, int pinned);
/* the launch scratch of `stream` on this context, at least `bytes`. A later request of no more
 * bytes for the same stream returns the same allocation, so a caller that asks for a launch's
 * scratch plus room of its own finds that room behind the launch's part */
void* bhrt_stream_scratch(devctx_t* c, hipStream_t stream, size_t bytes);
/* a second block of `stream`, with the same rule, that no bhrt_stream_scratch request moves */
void* bhrt_stream_keep(devctx_t* c, hipStream_t stream, size_t bytes);
/* One timed launch with a control block of the ring (kp->ctl, zero at launch; its counters
 * ctl[1..5] are folded into bhrt_stats): the trace kernel (fn NULL), or fn -- a launcher with
 * bhrt_launch_trace's contract and one more argument, named only by the file that passes it, so
 * the files of HOST_CORE link against stubs of the trace, path and particle launchers alone */
typedef int (*bhrt_launch_fn)(const bhrt_kparams* kp, const void* arg, void* stream, void* ev0,
                              void* ev1);
int bhrt_ctx_launch_fn(devctx_t* c, bhrt_kparams* kp, hipStream_t stream, bhrt_launch_fn fn,
                       const void* arg);
/* the NULL hip_stream of the device API */
int bhrt_null_unordered(void);
int bhrt_null_fence(devctx_t* c, int after);
typedef int (*bhrt_stream_body)(devctx_t* c, hipStream_t st, const void* arg);
int bhrt_on_stream(devctx_t* c, hipStream_t stream, bhrt_stream_body body, const void* arg);
void bhrt_drain_devices(int ndev);

/* ---- scene.c ---- */
int bhrt_check_scene(const BlackHoleParams* bh, const SimulationConfig* cfg);
int bhrt_fill_scene(bhrt_kparams* kp, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                    const SimulationConfig* cfg, IntegrationMethod method, int flags);
void bhrt_fill_camera(bhrt_kparams* kp, const bhrt_camera* cam, int W, int H);
void bhrt_fill_origin(bhrt_kparams* kp, const Vector3D* origin);
/* The thread's bound sky map (sky.c binds, bhrt_fill_scene copies it into a launch with
 * BHRT_FLAG_SKY): bind k's record for `device` (NULL unbinds); the bound texels or NULL; and the
 * refusal of a launch on `device` -- 0, or -1 with the error set where flags has BHRT_FLAG_SKY and
 * no map is bound or the bound one lives on another device. No HIP call. bhrt_fill_scene makes
 * that check for the current device and returns -1 the same way. */
void bhrt_sky_bind(const bhrt_sky_k* k, int device);
const void* bhrt_sky_bound(void);
int bhrt_sky_check(int flags, int device);
/* whether the trace kernel writes this scene's colour outputs */
int bhrt_colour_fused(int method, int has_disk, int spin);
int bhrt_colour_args_bad(const bhrt_frame_soa* out, int method, int has_disk, int spin);

/* ---- bhrt_api.c ---- */
/* bhrt_frame_soa as 15 pointers: the element size of each, and the one implementation of "sum
 * and carve 256-byte-aligned planes of n elements for the non-NULL fields" */
#define BHRT_NFIELDS 15
_Static_assert(sizeof(bhrt_frame_soa) == BHRT_NFIELDS * sizeof(void*), "bhrt_frame_soa fields");
static const size_t k_fsize[BHRT_NFIELDS] = {4, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 16, 4};
static inline void** soa_slot(bhrt_frame_soa* s, int f) { return ((void**)s) + f; }
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t bhrt_soa_bytes(const bhrt_frame_soa* fields, long n);
void bhrt_soa_carve(char** p, const bhrt_frame_soa* fields, long n, bhrt_frame_soa* dev);
bhrt_frame_soa bhrt_device_fields(const bhrt_frame_soa* want_in, int method, int has_disk,
                                  int spin);
/* bhrt_render_frame_device / bhrt_trace_rays_device on `stream` without the NULL-stream rule */
int bhrt_frame_on_device(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                         const SimulationConfig* cfg, const bhrt_camera* cam, int W, int H,
                         const bhrt_rows* rows, IntegrationMethod method, int flags,
                         const bhrt_frame_soa* out, hipStream_t stream, int use_order);
int bhrt_rays_on_device(const Ray* d_rays, const double* d_dirs, int n,
                        const BlackHoleParams* bh, const AccretionDiskParams* dk,
                        const SimulationConfig* cfg, IntegrationMethod method, int flags,
                        const bhrt_frame_soa* out, hipStream_t stream, const Vector3D* origin);

/* ---- supersample.c ---- */
typedef struct { /* a checked frame: shard pixels, samples per pixel and their offsets */
    int n, samples;
    double off_x[BHRT_SS_MAX_SAMPLES], off_y[BHRT_SS_MAX_SAMPLES];
} bhrt_ss_plan;
/* a supersampled frame's arguments (bhrt_render_frame_ss_device's refusals): 0 and the plan, or
 * -1 with the error set; no HIP call */
int bhrt_ss_check(const BlackHoleParams* bh, const SimulationConfig* cfg, const bhrt_camera* cam,
                  int W, int H, const bhrt_rows* rows, const SupersamplingParams* ss,
                  const AdaptiveSamplingParams* as, const bhrt_frame_soa* out, bhrt_ss_plan* k);

/* ---- kerr.c ---- */
/* The checks and set-up the Kerr calls share (the refusals of include/bhrt_api.h "Physical
 * geodesics"), each 0 or -1 with the error set and no HIP call beyond the current device's query:
 * the scene's constants; the output struct and flags; a ray array's arguments (both of the former,
 * n and rays); whether `o` has a static observer (i: the ray's index for the message, -1 none). */
int bhrt_kerr_scene(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                    const SimulationConfig* cfg, bhrt_kerr_k* k);
int bhrt_kerr_out_bad(const bhrt_frame_soa* out, int flags);
int bhrt_kerr_rays_check(const Ray* rays, int n, const BlackHoleParams* bh,
                         const AccretionDiskParams* dk, const SimulationConfig* cfg, int flags,
                         const bhrt_frame_soa* out, bhrt_kerr_k* k);
int bhrt_kerr_observer(const bhrt_kerr_k* k, const Vector3D* o, long i);
/* a camera call's own arguments -- the camera, the size, the row shard -- refused under the
 * family's prefix `who` ("kerr", "kerr_rk45", "kerr_emit"): 0 and the shard's rows, or -1 */
int bhrt_kerr_frame_check(const char* who, const bhrt_camera* cam, int W, int H,
                          const bhrt_rows* rows, int* nrows);
/* One checked launch of a frame / ray-array tracer (kerr.c, kerr_rk45.c, kerr_emit.c), for its
 * run under the stream rule: what the three families share. A family with more arguments puts
 * this first in a struct of its own. */
typedef struct {
    const BlackHoleParams* bh;
    const AccretionDiskParams* dk;
    const SimulationConfig* cfg;
    const bhrt_camera* cam; /* NULL: a ray array */
    int W, H, nrows;
    const bhrt_rows* rows;
    const Ray* d_rays;
    int n;
    int flags;
    const bhrt_frame_soa* out;
    double *h_residual, *lz_drift; /* the diagnostics' planes or NULL */
    const bhrt_kerr_k* k;
} bhrt_kerr_call;
/* kp and the bhrt_kerr_k part of the launch's second argument from the call: the colour's scene
 * and sky map, the camera (rows, tiles) or the rays, the outputs, the diagnostics' pointers. -1
 * with the error set where bhrt_fill_scene refuses. */
int bhrt_kerr_fill(const bhrt_kerr_call* a, bhrt_kparams* kp, bhrt_kerr_k* k);
/* The host forms' staging. A family's planes beside the bhrt_frame_soa fields are rows of a table,
 * in the order of their places in the context's buffer and of their copies. */
typedef struct {
    void* host;   /* the caller's array; NULL: not asked for (its place is kept, no copy is made) */
    void* dev;    /* the address of a pointer VARIABLE (a double* or int* object, never an integer
                   * or a struct) that is set to the device plane, or to NULL where host is NULL;
                   * it is written and read as bytes (memcpy), whatever its pointee type */
    size_t bytes;
    int preload;  /* the kernel writes only part of it: the device plane starts from `host` */
} bhrt_kerr_plane;
/* the pieces (kerr_paths.c stages its paths itself around them): the buffer bytes of the fields
 * asked for in hout and of every plane; their carving from *p with the uploads of sky_* and of the
 * preload planes on st; the copies back after the stream was synchronised */
size_t bhrt_kerr_stage_bytes(const bhrt_frame_soa* hout, long n, const bhrt_kerr_plane* pl,
                             int npl);
int bhrt_kerr_stage_carve(char** p, hipStream_t st, const bhrt_frame_soa* hout, long n,
                          bhrt_frame_soa* dout, const bhrt_kerr_plane* pl, int npl);
int bhrt_kerr_stage_back(const bhrt_frame_soa* hout, long n, const bhrt_frame_soa* dout,
                         const bhrt_kerr_plane* pl, int npl);
/* a whole host form: `a` with the host out and n rays in all -- `rays` on the host, or NULL for a
 * camera call. Sizes and carves the context's buffer, uploads the rays, runs body(c, st, arg) with
 * a->d_rays, a->out and the planes' pointers set to the device's, synchronises and copies back. */
int bhrt_kerr_host(bhrt_kerr_call* a, const Ray* rays, long n, const bhrt_kerr_plane* pl, int npl,
                   bhrt_stream_body body, const void* arg);
/* bhrt_kerr_rays_device's launch for arguments that passed bhrt_kerr_rays_check (k: its
 * constants), on `st` of context c without the NULL-stream rule */
int bhrt_kerr_rays_on_device(devctx_t* c, hipStream_t st, const Ray* d_rays, int n,
                             const BlackHoleParams* bh, const AccretionDiskParams* dk,
                             const SimulationConfig* cfg, int flags, const bhrt_frame_soa* out,
                             const bhrt_kerr_diag* diag, const bhrt_kerr_k* k);

/* ---- host_frames.c ---- */
typedef struct {
    devctx_t* c;
    bhrt_frame_soa dev;
    long n;
} shard_job;
int bhrt_host_threads(void);
/* n rows of P `elem`-byte points from a device rectangle to the caller's, count[i] points of row
 * i and nothing beyond them (the host forms of the path calls): 0, or -1 with the error set */
int bhrt_rows_back(void* host, const void* dev, const int32_t* count, int n, size_t P, size_t elem);

/* ---- dropin.c ---- */
struct BHContext_t { /* BHContextHandle (blackhole_api.c:26-31) */
    BlackHoleParams blackhole;
    AccretionDiskParams disk;
    SimulationConfig config;
    int disk_enabled;
};
/* generate_jittered_position (raytracer.c:868-932) */
void bhrt_jitter(int sample, int spp, JitterMethod jm, double strength, double* ox, double* oy);

#endif
