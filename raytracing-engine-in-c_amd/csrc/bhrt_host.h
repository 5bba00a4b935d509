/*
 * bhrt_host.h -- internals shared by the C host files of libbhrt.so (bhrt_api.c,
 * particles.c, supersample.c, paths.c). Not installed; hidden visibility.
 */
#ifndef BHRT_HOST_H
#define BHRT_HOST_H

#include <stddef.h>

#include "../../include/bhrt_api.h"
#include "bhrt_kernel.h"

/* per-thread error message read back by bhrt_last_error() */
void bhrt_set_err(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

/* BHContextHandle (blackhole_api.c:26-31) */
struct BHContext_t {
    BlackHoleParams blackhole;
    AccretionDiskParams disk;
    SimulationConfig config;
    int disk_enabled;
};

/* ---- bhrt_api.c internals that supersample.c builds on (thin wrappers of the static
 * functions named; a context is the calling thread's state of one device) ---- */
/* ctx_get(current device); NULL with the error set */
void* bhrt_hook_ctx(void);
/* ctx_streams + the context's own launch stream (a hipStream_t); NULL with the error set */
void* bhrt_hook_ctx_stream(void* ctx);
/* stream_scratch: the launch scratch of `stream` on this context, at least `bytes`. A later
 * request of no more bytes for the same stream returns the same allocation, so a caller that
 * asks for a launch's scratch plus room of its own finds that room behind the launch's part */
void* bhrt_hook_scratch(void* ctx, void* stream, size_t bytes);
/* a cached device buffer of the context for the outputs of bhrt_render_frame_ss and the arrays
 * of bhrt_trace_paths (calls that return only once their host arrays are complete) */
void* bhrt_hook_ss_buffer(void* ctx, size_t bytes);
/* null_unordered / null_fence: the NULL hip_stream of the device API */
int bhrt_hook_null_unordered(void);
int bhrt_hook_null_fence(void* ctx, int after);
/* trace_rays_device(NULL, d_dirs, ...): n packed directions (stride 3) from one origin */
int bhrt_hook_trace_dirs(const double* d_dirs, int n, const BlackHoleParams* bh,
                         const AccretionDiskParams* dk, const SimulationConfig* cfg,
                         IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                         void* stream, const Vector3D* origin);
/* trace_rays_device(d_rays, NULL, ...) on `stream` (not NULL): bhrt_trace_rays_device without
 * the NULL-stream fences */
int bhrt_hook_trace_rays(const Ray* d_rays, int n, const BlackHoleParams* bh,
                         const AccretionDiskParams* dk, const SimulationConfig* cfg,
                         IntegrationMethod method, int flags, const bhrt_frame_soa* out,
                         void* stream);
/* fill_scene then fill_camera */
void bhrt_hook_fill_camera(bhrt_kparams* kp, const BlackHoleParams* bh,
                           const AccretionDiskParams* dk, const SimulationConfig* cfg,
                           IntegrationMethod method, int flags, const bhrt_camera* cam, int W,
                           int H);
/* check_scene then fill_scene: 0, or -1 with the error set */
int bhrt_hook_scene(bhrt_kparams* kp, const BlackHoleParams* bh, const AccretionDiskParams* dk,
                    const SimulationConfig* cfg, IntegrationMethod method, int flags);
/* launch with another kernel's launcher: kp gets a control block of the context's ring (ctl,
 * zero at launch; its counters ctl[1..5] are folded into bhrt_stats as a trace launch's) and fn
 * runs between the launch's timing events. fn has bhrt_launch_trace's contract with one more
 * argument; bhrt_api.c never names the launcher itself (tests/fakehip) */
typedef int (*bhrt_launch_fn)(const bhrt_kparams* kp, const void* arg, void* stream, void* ev0,
                              void* ev1);
int bhrt_hook_launch(void* ctx, bhrt_kparams* kp, void* stream, bhrt_launch_fn fn,
                     const void* arg);
/* colour_fused: whether the trace kernel writes this scene's colour outputs */
int bhrt_hook_colour_fused(int method, int has_disk, int spin);
/* jitter: generate_jittered_position (raytracer.c:868-932) */
void bhrt_hook_jitter(int sample, int spp, JitterMethod jm, double strength, double* ox,
                      double* oy);

#endif
