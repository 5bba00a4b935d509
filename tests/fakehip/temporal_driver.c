/* temporal_driver.c -- the host side of temporal accumulation (temporal.c, over supersample.c's
 * sample offsets and the HOST_CORE files) on a SIMULATED device (fake_hip.c), built by
 * tests/test_temporal_cpu.py under ASan+UBSan as a stand-alone program.
 *
 * The launchers are stubs that check every launch buffer against the simulated device and fill
 * the device arrays from host code: the trace checks the camera's offset against the sample the
 * step must use and writes an encoding of (step, pixel, channel) into the scratch frame; the blend
 * stub checks that the scratch frame still holds that step's encoding (it survived until its
 * blend), its alpha, w and zero flag against the schedule, and blends in float; the edge stub
 * checks that it follows its step's blend and stamps the step into the edge array. main() walks
 * 40 frames with two resets through whole images and shards, on a stream and on the NULL stream,
 * through the device form, the caller-frame form and the host form, checks the state after every
 * call, the refusals, and that destroy frees what create allocated. Test infrastructure only. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "bhrt_api.h"
#include "bhrt_kernel.h"

int fakehip_kind_of(const void* p, size_t n);
int fakehip_current_device(void);

static int g_fail;
#define CHECK(x, ...)                                                            \
    do {                                                                         \
        if (!(x)) {                                                              \
            fprintf(stderr, "CHECK failed %s:%d: %s: ", __FILE__, __LINE__, #x); \
            fprintf(stderr, __VA_ARGS__);                                        \
            fputc('\n', stderr);                                                 \
            g_fail++;                                                            \
        }                                                                        \
    } while (0)
#define DIE(...)                      \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        fputc('\n', stderr);          \
        abort();                      \
    } while (0)

static void on_device(const void* p, size_t n, const char* what) {
    if (!p) DIE("launch buffer %s is NULL", what);
    const int k = fakehip_kind_of(p, n);
    if (k != fakehip_current_device())
        DIE("launch buffer %s (%zu B) is memory kind %d, launching on device %d", what, n, k,
            fakehip_current_device());
}

/* ---- what the next step must look like (set by main before each call) ---- */
static struct {
    int W, H, n, sharded;
    bhrt_rows rows;
    int render;            /* a trace belongs to the step */
    double off_x, off_y;   /* its offset */
    float alpha;
    int zero;
    int edges;             /* the edge launch belongs to the step */
    float threshold, decay;
    const float* caller;   /* the caller's frame (blend form) */
    const bhrt_accum_out* out; /* NULL: not checked (host form: the library's own buffers) */
    const float *acc, *edge;   /* the accumulator's arrays */
} g_want;
static int g_step;             /* steps made so far: the encoding's step */
static int g_phase;            /* 0 nothing yet, 1 traced, 2 blended, 3 edges done */
static const float* g_scratch; /* where this step's trace wrote */
static long g_traces, g_trace_rays, g_blends, g_edge_launches;

static float enc(int step, long i, int c) { return (float)((step % 50) * 0.015625 + (i % 97) * 0.001 + c * 0.1); }

int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    if (!g_want.render || g_phase != 0) DIE("trace launch in phase %d of step %d", g_phase, g_step);
    const size_t n = (size_t)kp->n;
    if (kp->n != g_want.n || kp->src != BHRT_SRC_CAMERA)
        DIE("trace launch of %d rays (src %d), want %d camera rays", kp->n, kp->src, g_want.n);
    if (kp->cam.width != g_want.W || kp->cam.height != g_want.H)
        DIE("trace launch of a %d x %d image", kp->cam.width, kp->cam.height);
    if (g_want.sharded && (kp->cam.rows.row_block != g_want.rows.row_block ||
                           kp->cam.rows.shard != g_want.rows.shard ||
                           kp->cam.rows.num_shards != g_want.rows.num_shards))
        DIE("trace launch without the shard");
    if (!g_want.sharded && kp->cam.rows.num_shards > 1) DIE("a whole image traced as a shard");
    if (kp->cam.off_x != g_want.off_x || kp->cam.off_y != g_want.off_y)
        DIE("step %d traced at offset (%.17g, %.17g), want (%.17g, %.17g)", g_step, kp->cam.off_x,
            kp->cam.off_y, g_want.off_x, g_want.off_y);
    on_device(kp->init, (size_t)(BHRT_INIT_FIELDS + 1) * 8 * n, "launch scratch");
    on_device(kp->ctl, 8 * 8, "control block");
    on_device(kp->out.rgba32f, 16 * n, "scratch frame");
    void* const* f = (void* const*)&kp->out;
    for (int i = 0; i < 15; i++)
        if (f[i] && (const void*)f[i] != (const void*)kp->out.rgba32f)
            DIE("trace launch writes field %d besides rgba32f", i);
    memset(kp->init, 0x5a, (size_t)(BHRT_INIT_FIELDS + 1) * 8 * n); /* (the kernel's own use) */
    for (size_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++) kp->out.rgba32f[4 * i + c] = enc(g_step, (long)i, c);
        kp->out.rgba32f[4 * i + 3] = 1.0f;
    }
    g_scratch = kp->out.rgba32f;
    kp->ctl[1] += n;
    g_traces++;
    g_trace_rays += (long)n;
    g_phase = 1;
    return 0;
}

int bhrt_launch_ta_blend(const bhrt_ta_blend_k* k, void* stream) {
    (void)stream;
    if (g_phase != (g_want.render ? 1 : 0)) DIE("blend launch in phase %d of step %d", g_phase, g_step);
    const size_t n = (size_t)k->n;
    if (k->n != g_want.n) DIE("blend launch of %ld pixels, want %d", k->n, g_want.n);
    if (k->stride != (g_want.render ? 4 : 3)) DIE("blend launch with stride %d", k->stride);
    on_device(k->frame, 4 * (size_t)k->stride * n, "new frame");
    on_device(k->acc, 12 * n, "acc");
    if (k->acc != g_want.acc) DIE("blend launch on another acc array");
    if (g_want.render) {
        if (k->frame != g_scratch) DIE("blend reads %p, the trace wrote %p", (const void*)k->frame, (const void*)g_scratch);
        for (size_t i = 0; i < n; i++)  /* the scratch frame survived until its blend */
            for (int c = 0; c < 3; c++)
                if (k->frame[4 * i + c] != enc(g_step, (long)i, c))
                    DIE("step %d: scratch frame lost pixel %zu channel %d: %g", g_step, i, c,
                        (double)k->frame[4 * i + c]);
    } else if (k->frame != g_want.caller) {
        DIE("blend launch does not read the caller's frame");
    }
    if (k->alpha != g_want.alpha || k->w != 1.0f - g_want.alpha || k->zero != g_want.zero)
        DIE("step %d: alpha %g w %g zero %d, want alpha %g zero %d", g_step, (double)k->alpha,
            (double)k->w, k->zero, (double)g_want.alpha, g_want.zero);
    if (g_want.out) {
        if (k->rgb != g_want.out->rgb || k->rgba8 != g_want.out->rgba8)
            DIE("blend launch does not write the caller's outputs");
    }
    if (k->rgb) on_device(k->rgb, 12 * n, "rgb copy");
    if (k->rgba8) on_device(k->rgba8, 4 * n, "rgba8");
    for (size_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++) {
            const float old = k->zero ? 0.0f : k->acc[3 * i + c];
            const float v = old * k->w + k->frame[(size_t)k->stride * i + c] * k->alpha;
            k->acc[3 * i + c] = v;
            if (k->rgb) k->rgb[3 * i + c] = v;
        }
        if (k->rgba8) {
            k->rgba8[4 * i] = (uint8_t)(g_step % 251);
            k->rgba8[4 * i + 3] = 255;
        }
    }
    g_blends++;
    g_phase = 2;
    return 0;
}

int bhrt_launch_ta_edges(const bhrt_ta_edges_k* k, void* stream) {
    (void)stream;
    if (g_phase != 2 || !g_want.edges) DIE("edge launch in phase %d of step %d", g_phase, g_step);
    const size_t n = (size_t)k->n;
    if (k->n != g_want.n || k->width != g_want.W || k->height != g_want.H)
        DIE("edge launch of %ld pixels (%d x %d)", k->n, k->width, k->height);
    if (k->threshold != g_want.threshold || k->decay != g_want.decay)
        DIE("edge launch with threshold %g decay %g", (double)k->threshold, (double)k->decay);
    on_device(k->acc, 12 * n, "acc");
    on_device(k->edge, 4 * n, "edge");
    if (k->acc != g_want.acc || k->edge != g_want.edge) DIE("edge launch on other arrays");
    if (g_want.out && k->out != g_want.out->edge_factor) DIE("edge launch: wrong output array");
    if (k->out) on_device(k->out, 4 * n, "edge_factor");
    for (size_t i = 0; i < n; i++) {
        if (g_step == 0 && k->edge[i] != 0.0f) DIE("edge[%zu] is %g at the first step", i, (double)k->edge[i]);
        k->edge[i] = (float)(g_step + 1);
        if (k->out) k->out[i] = k->edge[i];
    }
    g_edge_launches++;
    g_phase = 3;
    return 0;
}

/* the launchers the linked files name besides; none is reached here */
int bhrt_launch_ss_rays(const bhrt_ss_rays_k* k, void* s) { (void)k; (void)s; return 100; }
int bhrt_launch_ss_resolve(const bhrt_ss_resolve_k* k, void* s) { (void)k; (void)s; return 100; }
int bhrt_launch_path(const bhrt_kparams* kp, const double* o, const double* d, Vector3D* p,
                     int m, int* nn, int nin, void* st) {
    (void)kp; (void)o; (void)d; (void)p; (void)m; (void)nn; (void)nin; (void)st;
    return 100;
}
int bhrt_launch_particles(Particle* d, int count, const bhrt_particle_k* k, int steps,
                          void* stream, void* ev0, void* ev1) {
    (void)d; (void)count; (void)k; (void)steps; (void)stream; (void)ev0; (void)ev1;
    return 100;
}

/* ---- the scene ---- */
static BlackHoleParams g_bh;
static AccretionDiskParams g_dk;
static SimulationConfig g_cfg;
static bhrt_camera g_cam;

static void scene(void) {
    initialize_black_hole_params(&g_bh, 1.0, 0.0, 0.0);
    const AccretionDiskParams d = {6.0, 20.0, 1.0, 1.0, 0.0, 0.0};
    g_dk = d;
    memset(&g_cfg, 0, sizeof g_cfg);
    g_cfg.time_step = 0.1;
    g_cfg.max_ray_distance = 100.0;
    g_cfg.max_integration_steps = 100;
    g_cfg.tolerance = 1e-6;
    memset(&g_cam, 0, sizeof g_cam);
    g_cam.position.z = 30.0;
    g_cam.position.y = 3.0;
    g_cam.direction.z = -1.0;
    g_cam.up.y = 1.0;
    g_cam.fov_deg = 40.0;
}

static float want_alpha(const bhrt_accum_params* p, int fc) {
    if (p->schedule == BHRT_ACCUM_MEAN) return 1.0f / (float)(fc + 1);
    return fc == 0 ? 1.0f : (fc < 5 ? 0.5f : p->blend_factor);
}

/* One accumulator through `frames` steps with resets before steps 17 and 31: form 0 = device
 * frames, 1 = caller frames, 2 = host frames. */
static void run(int W, int H, const bhrt_rows* rows, const bhrt_accum_params* par, int spp,
                JitterMethod jm, int form, hipStream_t stream, int frames) {
    char what[128];
    snprintf(what, sizeof what, "%dx%d shard %d/%d schedule %d spp %d form %d%s", W, H,
             rows ? rows->shard : 0, rows ? rows->num_shards : 1, par ? par->schedule : 0, spp, form,
             stream ? "" : " NULL stream");
    const bhrt_accum_params dflt = {BHRT_ACCUM_REFERENCE, 0.1f, 32, 0.1f, 0.2f};
    const bhrt_accum_params p = par ? *par : dflt;
    SupersamplingParams ss;
    memset(&ss, 0, sizeof ss);
    ss.samples_per_pixel = spp;
    ss.jitter_method = jm;
    ss.jitter_strength = 1.0;
    const SupersamplingParams* pss = spp > 0 ? &ss : NULL;
    double ox[BHRT_SS_MAX_SAMPLES], oy[BHRT_SS_MAX_SAMPLES];
    const int cycle = form == 1 ? BHRT_SS_MAX_SAMPLES
                                : bhrt_sample_offsets(pss, NULL, ox, oy, BHRT_SS_MAX_SAMPLES);
    if (cycle < 1) DIE("%s: sample offsets: %s", what, bhrt_last_error());
    bhrt_accum* a = NULL;
    if (bhrt_accum_create(W, H, rows, par, &a) != 0 || !a) DIE("%s: create: %s", what, bhrt_last_error());
    memset(&g_want, 0, sizeof g_want);
    g_want.W = W;
    g_want.H = H;
    g_want.sharded = rows && rows->num_shards > 1;
    if (rows) g_want.rows = *rows;
    g_want.n = bhrt_shard_rows(H, rows) * W;
    const size_t n = (size_t)g_want.n, n1 = n ? n : 1;
    CHECK(bhrt_accum_device_buffers(a, &g_want.acc, &g_want.edge) == 0, "%s: buffers", what);
    if (n) {
        on_device(g_want.acc, 12 * n, "acc");
        on_device(g_want.edge, 4 * n, "edge");
        for (size_t i = 0; i < 3 * n; i++)
            if (g_want.acc[i] != 0.0f) DIE("%s: acc not zero at creation", what);
        for (size_t i = 0; i < n; i++)
            if (g_want.edge[i] != 0.0f) DIE("%s: edge not zero at creation", what);
    }
    bhrt_accum_out out;
    memset(&out, 0, sizeof out);
    float* d_frame = NULL;
    float* mirror = (float*)calloc(3 * n1, sizeof(float)); /* the rule's acc on the host */
    if (form != 2) {
        if (hipMalloc((void**)&out.rgba8, 4 * n1) || hipMalloc((void**)&out.rgb, 12 * n1) ||
            hipMalloc((void**)&d_frame, 12 * n1))
            DIE("hipMalloc failed");
        if (!g_want.sharded && hipMalloc((void**)&out.edge_factor, 4 * n1)) DIE("hipMalloc failed");
    } else { /* exact-size host arrays: ASan sees one element too many */
        out.rgba8 = (uint8_t*)malloc(4 * n1);
        out.rgb = (float*)malloc(12 * n1);
        if (!g_want.sharded) out.edge_factor = (float*)malloc(4 * n1);
    }
    int fc = 0, ji = 0, pending = 1;
    long total = 0;
    g_step = 0;
    for (int k = 0; k < frames; k++) {
        if (k == 17 || k == 31) {
            CHECK(bhrt_accum_reset(a) == 0, "%s: reset", what);
            pending = 1;
        }
        bhrt_accum_state s;
        CHECK(bhrt_accum_info(a, form == 1 ? NULL : pss, &s) == 0, "%s: info: %s", what, bhrt_last_error());
        const float al = want_alpha(&p, pending ? 0 : fc);
        CHECK(s.frame_count == fc && s.jitter_index == ji && s.reset_pending == pending &&
                  s.frames_total == total && s.pixels == (int64_t)n && s.next_alpha == al &&
                  s.sharded == g_want.sharded,
              "%s: state before step %d: fc %d ji %d pending %d total %lld alpha %g", what, k,
              s.frame_count, s.jitter_index, s.reset_pending, (long long)s.frames_total,
              (double)s.next_alpha);
        if (form != 1)
            CHECK(s.cycle == cycle && s.next_offset_x == ox[ji % cycle] &&
                      s.next_offset_y == oy[ji % cycle],
                  "%s: next offset before step %d", what, k);
        g_want.render = form != 1;
        g_want.off_x = form != 1 ? ox[ji % cycle] : 0.0;
        g_want.off_y = form != 1 ? oy[ji % cycle] : 0.0;
        g_want.alpha = al;
        g_want.zero = pending;
        g_want.edges = !g_want.sharded && p.edge_threshold == p.edge_threshold;
        g_want.threshold = p.edge_threshold;
        g_want.decay = p.edge_decay;
        g_want.caller = d_frame;
        g_want.out = form == 2 ? NULL : &out;
        g_phase = 0;
        if (form == 1)
            for (size_t i = 0; i < n; i++)
                for (int c = 0; c < 3; c++) d_frame[3 * i + c] = enc(k, (long)i, c);
        int rc;
        if (form == 0)
            rc = bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, pss,
                                         &out, stream);
        else if (form == 1)
            rc = bhrt_accum_blend_device(a, d_frame, &out, stream);
        else
            rc = bhrt_accum_frame(a, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, pss, &out);
        CHECK(rc == 0, "%s: step %d rc %d (%s)", what, k, rc, bhrt_last_error());
        if (rc != 0) break;
        if (n) CHECK(g_phase == (g_want.edges ? 3 : 2), "%s: step %d ended in phase %d", what, k, g_phase);
        if (pending) fc = 0, pending = 0;
        fc = fc + 1 < p.max_frames ? fc + 1 : p.max_frames;
        ji = (ji % cycle + 1) % cycle;
        total++;
        for (size_t i = 0; i < n; i++)
            for (int c = 0; c < 3; c++) {
                const float old = g_want.zero ? 0.0f : mirror[3 * i + c];
                mirror[3 * i + c] = old * (1.0f - al) + enc(k, (long)i, c) * al;
                if (out.rgb[3 * i + c] != mirror[3 * i + c] || g_want.acc[3 * i + c] != mirror[3 * i + c])
                    DIE("%s: step %d pixel %zu channel %d: rgb %g acc %g, want %g", what, k, i, c,
                        (double)out.rgb[3 * i + c], (double)g_want.acc[3 * i + c], (double)mirror[3 * i + c]);
            }
        for (size_t i = 0; i < n; i++) {
            if (out.rgba8[4 * i] != (uint8_t)(k % 251) || out.rgba8[4 * i + 3] != 255)
                DIE("%s: step %d rgba8 of pixel %zu", what, k, i);
            if (out.edge_factor) {
                const float e = g_want.edges ? (float)(k + 1) : 0.0f;
                if (out.edge_factor[i] != e) DIE("%s: step %d edge_factor[%zu] = %g, want %g", what, k, i, (double)out.edge_factor[i], (double)e);
            }
        }
        g_step++;
    }
    /* the refusals of a live accumulator: nothing launched, the state as it was */
    bhrt_accum_state s0, s1;
    CHECK(bhrt_accum_info(a, NULL, &s0) == 0, "%s: info", what);
    g_want.render = 0;
    g_phase = 7; /* any launch now dies in its stub */
    bhrt_camera off = g_cam;
    off.use_offset = 1;
    SupersamplingParams rnd = ss;
    rnd.samples_per_pixel = 4;
    rnd.jitter_method = JITTER_RANDOM;
    SupersamplingParams many = ss;
    many.samples_per_pixel = 65;
    many.jitter_method = JITTER_HALTON;
    float dummy = 0.0f;
    bhrt_accum_out shard_edges = {NULL, NULL, &dummy};
    CHECK(bhrt_accum_frame_device(a, NULL, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, pss, &out, stream) == -1, "%s: NULL blackhole", what);
    CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, NULL, &g_cam, INTEGRATOR_RK4, 0, pss, &out, stream) == -1, "%s: NULL config", what);
    CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, NULL, INTEGRATOR_RK4, 0, pss, &out, stream) == -1, "%s: NULL camera", what);
    CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, pss, NULL, stream) == -1, "%s: NULL out", what);
    CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, &off, INTEGRATOR_RK4, 0, pss, &out, stream) == -1, "%s: use_offset", what);
    CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, &rnd, &out, stream) == -1, "%s: random jitter", what);
    CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, &many, &out, stream) == -1, "%s: 65 samples", what);
    CHECK(bhrt_accum_blend_device(a, NULL, &out, stream) == -1, "%s: NULL frame", what);
    if (g_want.sharded) {
        CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, pss, &shard_edges, stream) == -1, "%s: edge_factor of a shard", what);
        CHECK(strstr(bhrt_last_error(), "edge_factor") != NULL, "%s: message %s", what, bhrt_last_error());
        CHECK(bhrt_accum_blend_device(a, d_frame ? d_frame : &dummy, &shard_edges, stream) == -1, "%s: edge_factor of a shard (blend)", what);
    }
    CHECK(dummy == 0.0f, "%s: a refused call wrote", what);
    CHECK(bhrt_accum_info(a, NULL, &s1) == 0 && memcmp(&s0, &s1, sizeof s0) == 0, "%s: a refused call moved the state", what);
    const void* base = g_want.acc;
    bhrt_accum_destroy(a);
    CHECK(fakehip_kind_of(base, 1) != fakehip_current_device(), "%s: destroy left the state arrays allocated", what);
    if (form != 2) {
        (void)hipFree(out.rgba8); (void)hipFree(out.rgb); (void)hipFree(out.edge_factor); (void)hipFree(d_frame);
    } else {
        free(out.rgba8); free(out.rgb); free(out.edge_factor);
    }
    free(mirror);
}

int main(void) {
    scene();
    hipStream_t st;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) DIE("stream");
    const bhrt_accum_params mean = {BHRT_ACCUM_MEAN, 0.1f, 32, 0.1f, 0.2f};
    const bhrt_accum_params other = {BHRT_ACCUM_REFERENCE, 0.25f, 8, 0.05f, 0.3f};
    const bhrt_accum_params noedge = {BHRT_ACCUM_REFERENCE, 0.1f, 32, NAN, 0.2f};
    const bhrt_rows s0 = {3, 0, 2}, s1 = {3, 1, 2}, s2 = {8, 2, 3}, none = {4, 2, 3};
    for (int form = 0; form < 3; form++) {
        run(7, 5, NULL, NULL, 8, JITTER_HALTON, form, st, 40);
        run(7, 5, NULL, &mean, 4, JITTER_REGULAR_GRID, form, NULL, 40);
        run(1, 1, NULL, &other, 0, JITTER_REGULAR_GRID, form, st, 40);
        run(5, 4, NULL, &noedge, 3, JITTER_HALTON, form, st, 40);
        run(6, 16, &s0, NULL, 4, JITTER_REGULAR_GRID, form, st, 40);
        run(6, 16, &s1, &mean, 8, JITTER_HALTON, form, NULL, 40);
        run(4, 40, &s2, &other, 1, JITTER_REGULAR_GRID, form, st, 40);
        run(3, 5, &none, NULL, 4, JITTER_REGULAR_GRID, form, st, 40); /* a shard without rows */
    }
    /* create's refusals: the handle untouched */
    bhrt_accum* h = (bhrt_accum*)&g_fail;
    const struct { bhrt_accum_params p; const char* what; } bad[] = {
        {{7, 0.1f, 32, 0.1f, 0.2f}, "schedule"},       {{0, NAN, 32, 0.1f, 0.2f}, "blend_factor"},
        {{0, -0.1f, 32, 0.1f, 0.2f}, "blend_factor"},  {{0, 1.5f, 32, 0.1f, 0.2f}, "blend_factor"},
        {{0, 0.1f, 0, 0.1f, 0.2f}, "max_frames"},      {{0, 0.1f, 32, 0.1f, -0.2f}, "edge_decay"},
        {{0, 0.1f, 32, 0.1f, NAN}, "edge_decay"}};
    for (size_t i = 0; i < sizeof bad / sizeof *bad; i++) {
        CHECK(bhrt_accum_create(4, 4, NULL, &bad[i].p, &h) == -1 && h == (bhrt_accum*)&g_fail,
              "create accepted a bad %s", bad[i].what);
        CHECK(strstr(bhrt_last_error(), bad[i].what) != NULL, "message for %s: %s", bad[i].what, bhrt_last_error());
    }
    const bhrt_rows badrows = {0, 0, 2};
    CHECK(bhrt_accum_create(0, 4, NULL, NULL, &h) == -1, "create accepted width 0");
    CHECK(bhrt_accum_create(4, -1, NULL, NULL, &h) == -1, "create accepted height -1");
    CHECK(bhrt_accum_create(4, 4, &badrows, NULL, &h) == -1, "create accepted bad rows");
    CHECK(bhrt_accum_create(65536, 65536, NULL, NULL, &h) == -1, "create accepted 2^32 pixels");
    CHECK(bhrt_accum_create(4, 4, NULL, NULL, NULL) == -1, "create accepted a NULL handle pointer");
    CHECK(h == (bhrt_accum*)&g_fail, "a refused create wrote the handle");
    CHECK(bhrt_accum_reset(NULL) == -1 && bhrt_accum_info(NULL, NULL, NULL) == -1 &&
              bhrt_accum_device_buffers(NULL, NULL, NULL) == -1, "NULL handles accepted");
    CHECK(bhrt_accum_frame_device(NULL, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, NULL, NULL, st) == -1, "NULL handle accepted");
    bhrt_accum_destroy(NULL);
    /* create / destroy: every allocation freed again */
    for (int i = 0; i < 200; i++) {
        bhrt_accum* a = NULL;
        const float *rgb = NULL, *edge = NULL;
        if (bhrt_accum_create(9, 9, NULL, NULL, &a) != 0) DIE("create %d: %s", i, bhrt_last_error());
        (void)bhrt_accum_device_buffers(a, &rgb, &edge);
        bhrt_accum_destroy(a);
        CHECK(fakehip_kind_of(rgb, 4) != fakehip_current_device(), "create/destroy %d leaked", i);
    }
    /* an accumulator is bound to the device it was made on */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 1) {
        bhrt_accum* a = NULL;
        float frame[3 * 4] = {0};
        bhrt_accum_out none_out = {NULL, NULL, NULL};
        if (bhrt_accum_create(2, 2, NULL, NULL, &a) != 0) DIE("create: %s", bhrt_last_error());
        g_phase = 7; /* any launch dies in its stub */
        g_want.render = 0;
        if (hipSetDevice(1) != hipSuccess) DIE("hipSetDevice(1)");
        CHECK(bhrt_accum_frame_device(a, &g_bh, &g_dk, &g_cfg, &g_cam, INTEGRATOR_RK4, 0, NULL, &none_out, st) == -1 &&
                  strstr(bhrt_last_error(), "current device") != NULL, "frame on another device: %s", bhrt_last_error());
        CHECK(bhrt_accum_blend_device(a, frame, NULL, st) == -1 &&
                  strstr(bhrt_last_error(), "current device") != NULL, "blend on another device: %s", bhrt_last_error());
        if (hipSetDevice(0) != hipSuccess) DIE("hipSetDevice(0)");
        bhrt_accum_state s;
        CHECK(bhrt_accum_info(a, NULL, &s) == 0 && s.frames_total == 0 && s.reset_pending == 1, "a refused call moved the state");
        bhrt_accum_destroy(a);
    } else {
        CHECK(0, "the driver needs two simulated devices (FAKEHIP_DEVICES=2)");
    }
    bhrt_stats stt;
    CHECK(bhrt_get_stats(&stt, 1) == 0, "stats: %s", bhrt_last_error());
    CHECK((long)stt.launches == g_traces && (long)stt.rays == g_trace_rays,
          "stats: %llu launches %llu rays, %ld and %ld made", (unsigned long long)stt.launches,
          (unsigned long long)stt.rays, g_traces, g_trace_rays);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld trace launches, %ld rays, %ld blends, %ld edge launches)\n",
           g_traces, g_trace_rays, g_blends, g_edge_launches);
    return 0;
}
