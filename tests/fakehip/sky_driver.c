/* sky_driver.c -- sky maps (sky.c over the HOST_CORE files) on SIMULATED devices (fake_hip.c),
 * built by tests/test_sky_cpu.py under ASan+UBSan as a stand-alone program.
 *
 * The launchers are stubs: the sky launcher checks the map it is given against the simulated
 * device -- the texels of both input formats as the 16-byte records the kernels read -- and fills
 * the colours with an encoding of the directions; the trace launcher records the sky block of
 * every launch. The HIP entry points the sky code can reach are counted through the linker's
 * --wrap, so "no HIP call" is checked, not assumed.
 *
 * Checked: every refusal of include/bhrt_api.h "Sky maps" with zero HIP calls (the current
 * device's query aside, for the one refusal that needs it) and nothing written; the upload of
 * both formats; the host lookup's round trip; a frame with the flag and no map bound; the block a
 * frame with a bound map carries, fused and with the separate colour pass; a bound map without
 * the flag; a map of a second device; the host form's and the gather's multi-device split;
 * destroy unbinds. Test infrastructure only. */
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

/* ---- HIP calls, counted (-Wl,--wrap=...) ---- */
static long g_hip, g_query;
#define WRAP(ret, name, params, args)  \
    ret __real_##name params;          \
    ret __wrap_##name params {         \
        g_hip++;                       \
        return __real_##name args;     \
    }
WRAP(hipError_t, hipMalloc, (void** p, size_t n), (p, n))
WRAP(hipError_t, hipFree, (void* p), (p))
WRAP(hipError_t, hipMemcpy, (void* d, const void* s, size_t n, hipMemcpyKind k), (d, s, n, k))
WRAP(hipError_t, hipMemcpyAsync, (void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st),
     (d, s, n, k, st))
WRAP(hipError_t, hipSetDevice, (int d), (d))
WRAP(hipError_t, hipStreamSynchronize, (hipStream_t s), (s))
WRAP(hipError_t, hipEventRecord, (hipEvent_t e, hipStream_t s), (e, s))
WRAP(hipError_t, hipStreamWaitEvent, (hipStream_t s, hipEvent_t e, unsigned f), (s, e, f))
WRAP(hipError_t, hipHostMalloc, (void** p, size_t n, unsigned f), (p, n, f))
hipError_t __real_hipGetDevice(int* d);
hipError_t __wrap_hipGetDevice(int* d) {
    g_query++;
    return __real_hipGetDevice(d);
}
/* (fake_hip.c has no device-wide wait: every simulated call completes at once) */
hipError_t hipDeviceSynchronize(void) {
    g_hip++;
    return hipSuccess;
}

static void on_device(const void* p, size_t n, const char* what) {
    const int k = fakehip_kind_of(p, n);
    if (k != fakehip_current_device()) {
        fprintf(stderr, "launch buffer %s (%zu B) is memory kind %d, launching on device %d\n",
                what, n, k, fakehip_current_device());
        abort();
    }
}

/* ---- launcher stubs ---- */
static long g_sky_launches, g_traces;
static const float* g_want_tex; /* the 16-byte records the next sky launch must find */
static bhrt_sky_k g_seen;       /* the sky block of the last trace launch */
static int g_seen_flags, g_seen_fused;

int bhrt_launch_sky(const bhrt_sky_k* sky, const double* d_dirs, int n, double* d_rgb,
                    void* stream) {
    (void)stream;
    const size_t texels = (size_t)sky->w * (size_t)sky->h;
    on_device(sky->tex, 16 * texels, "sky texels");
    on_device(d_dirs, 24 * (size_t)n, "directions");
    on_device(d_rgb, 24 * (size_t)n, "colours");
    CHECK(sky->chord == NULL, "a lookup launch with a chord scratch");
    CHECK(sky->sx == (double)sky->w / (2.0 * BH_PI) && sky->sy == (double)sky->h / BH_PI,
          "scale factors %g %g", sky->sx, sky->sy);
    if (g_want_tex)
        CHECK(memcmp(sky->tex, g_want_tex, 16 * texels) == 0, "texel records differ");
    for (int i = 0; i < 3 * n; i++) d_rgb[i] = d_dirs[i] * 2.0 + 1.0;
    g_sky_launches++;
    return 0;
}

int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    const size_t n = (size_t)kp->n;
    on_device(kp->ctl, 8 * 8, "control block");
    on_device(kp->init, (size_t)BHRT_SCRATCH_FIELDS * 8 * n, "launch scratch");
    if (kp->sky.tex) on_device(kp->sky.tex, 16 * (size_t)kp->sky.w * (size_t)kp->sky.h, "sky texels");
    if (kp->sky.chord) {
        on_device(kp->sky.chord, 24 * n, "chord scratch");
        CHECK(kp->sky.chord == kp->init + (size_t)(BHRT_INIT_FIELDS + 1) * n, "chord scratch place");
        CHECK((char*)kp->sky.chord >= (char*)kp->redo + 4 * n, "chord scratch overlaps the redo list");
    }
    g_seen = kp->sky;
    g_seen_flags = kp->sc.flags;
    g_seen_fused = kp->colour_fused;
    if (kp->out.rgba8) memset(kp->out.rgba8, 0x11, 4 * n);
    kp->ctl[1] += n;
    g_traces++;
    return 0;
}
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

/* ---- the scene of every frame ---- */
static BlackHoleParams bh;
static AccretionDiskParams dk = {6.0, 20.0, 1.0, 1.0, 0.0, 0.0};
static SimulationConfig cfg;
static bhrt_camera cam = {{0.0, -29.544, 5.209}, {0.0, 29.544, -5.209}, {0.0, 0.0, 1.0}, 60.0, 0, 0.0, 0.0};
enum { FW = 16, FH = 16 };

/* one device frame into a device rgba8 array (and what the separate pass reads); the rc */
static int frame(int flags, int separate, int* written) {
    bhrt_frame_soa out;
    memset(&out, 0, sizeof out);
    const size_t n = FW * FH;
    void *d8 = NULL, *dr = NULL, *dx = NULL, *dy = NULL;
    if (__real_hipMalloc(&d8, 4 * n) != hipSuccess) abort();
    memset(d8, 0x77, 4 * n);
    out.rgba8 = (uint8_t*)d8;
    if (separate) {
        if (__real_hipMalloc(&dr, 4 * n) || __real_hipMalloc(&dx, 8 * n) || __real_hipMalloc(&dy, 8 * n))
            abort();
        out.result = (int32_t*)dr;
        out.hit_x = (double*)dx;
        out.hit_y = (double*)dy;
    }
    const int rc = bhrt_render_frame_device(&bh, &dk, &cfg, &cam, FW, FH, NULL, INTEGRATOR_RK4,
                                            flags, &out, NULL);
    if (written) *written = ((unsigned char*)d8)[0] != 0x77;
    __real_hipFree(d8);
    if (dr) __real_hipFree(dr);
    if (dx) __real_hipFree(dx);
    if (dy) __real_hipFree(dy);
    return rc;
}

static int has(const char* needle) { return strstr(bhrt_last_error(), needle) != NULL; }

int main(void) {
    initialize_black_hole_params(&bh, 1.0, 0.0, 0.0);
    memset(&cfg, 0, sizeof cfg);
    cfg.time_step = 0.1;
    cfg.max_ray_distance = 100.0;
    cfg.max_integration_steps = 100;
    cfg.tolerance = 1e-6;

    /* exact-size host maps: ASan sees one element too many */
    enum { SW = 5, SH = 3, ST = SW * SH };
    float* f32 = (float*)malloc(ST * 3 * sizeof(float));
    unsigned char* u8 = (unsigned char*)malloc(ST * 4);
    float* want32 = (float*)malloc(ST * 16);
    float* want8 = (float*)malloc(ST * 16);
    for (int i = 0; i < ST; i++) {
        for (int c = 0; c < 3; c++) {
            f32[3 * i + c] = (float)(i * 3 + c) * 0.01f - 0.05f;
            want32[4 * i + c] = f32[3 * i + c];
            u8[4 * i + c] = (unsigned char)((i * 17 + c * 5) & 255);
            want8[4 * i + c] = (float)u8[4 * i + c] / 255.0f;
        }
        u8[4 * i + 3] = (unsigned char)i; /* alpha: ignored */
        want32[4 * i + 3] = want8[4 * i + 3] = 1.0f;
    }
    u8[4 * 2 + 0] = 255; /* (255 -> exactly 1.0f) */
    want8[4 * 2 + 0] = 1.0f;

    /* ---- 1. refusals without an object: zero HIP calls, not even the query; nothing written ---- */
    bhrt_sky* const poison = (bhrt_sky*)0x7777;
    bhrt_sky* h = poison;
    g_hip = g_query = 0;
    CHECK(bhrt_sky_create(NULL, SW, SH, BHRT_SKY_RGB32F, &h) == -1 && has("NULL"), "NULL texels");
    CHECK(bhrt_sky_create(f32, SW, SH, BHRT_SKY_RGB32F, NULL) == -1 && has("NULL"), "NULL handle");
    CHECK(bhrt_sky_create(f32, 0, SH, BHRT_SKY_RGB32F, &h) == -1 && has("invalid size"), "width 0");
    CHECK(bhrt_sky_create(f32, SW, -1, BHRT_SKY_RGB32F, &h) == -1 && has("invalid size"), "height -1");
    CHECK(bhrt_sky_create(f32, 8193, 8192, BHRT_SKY_RGB32F, &h) == -1 && has("2^26"), "too large");
    CHECK(bhrt_sky_create(f32, 1 << 30, 1 << 30, BHRT_SKY_RGBA8, &h) == -1 && has("2^26"), "2^60 texels");
    CHECK(bhrt_sky_create(f32, SW, SH, 2, &h) == -1 && has("unknown format"), "format 2");
    CHECK(bhrt_sky_create(f32, SW, SH, -1, &h) == -1 && has("unknown format"), "format -1");
    const float bad[3] = {NAN, INFINITY, -INFINITY};
    for (int b = 0; b < 3; b++) {
        const float keep = f32[3 * 7 + 1];
        f32[3 * 7 + 1] = bad[b];
        CHECK(bhrt_sky_create(f32, SW, SH, BHRT_SKY_RGB32F, &h) == -1 && has("not finite") &&
              has("(2, 1) channel 1"), "non-finite texel %d: %s", b, bhrt_last_error());
        f32[3 * 7 + 1] = keep;
    }
    bhrt_sky_state st = {7, 7, 7, 7};
    double io[6] = {1, 2, 3, 4, 5, 6};
    CHECK(bhrt_sky_info(NULL, &st) == -1 && st.width == 7, "info of NULL");
    CHECK(bhrt_sky_lookup(NULL, io, 1, io + 3) == -1 && has("NULL"), "lookup of NULL");
    CHECK(bhrt_sky_lookup_device(NULL, io, 1, io + 3, NULL) == -1 && has("NULL"), "device lookup of NULL");
    bhrt_sky_destroy(NULL);
    CHECK(h == poison && g_hip == 0 && g_query == 0, "refusals made %ld HIP calls, %ld queries", g_hip, g_query);

    /* ---- 2. both formats: the records on the device, the host lookup's round trip ---- */
    bhrt_sky *s32 = NULL, *s8 = NULL;
    CHECK(bhrt_sky_create(f32, SW, SH, BHRT_SKY_RGB32F, &s32) == 0 && s32, "create rgb32f: %s", bhrt_last_error());
    CHECK(bhrt_sky_create(u8, SW, SH, BHRT_SKY_RGBA8, &s8) == 0 && s8, "create rgba8: %s", bhrt_last_error());
    g_hip = g_query = 0;
    CHECK(bhrt_sky_info(s8, &st) == 0 && st.width == SW && st.height == SH &&
          st.format == BHRT_SKY_RGBA8 && st.device == 0 && g_hip == 0 && g_query == 0, "info");
    for (int n = 1; n <= 2; n++) {
        double* dirs = (double*)malloc(24 * (size_t)n);
        double* rgb = (double*)malloc(24 * (size_t)n);
        for (int i = 0; i < 3 * n; i++) {
            dirs[i] = i + 0.5;
            rgb[i] = -1.0;
        }
        g_want_tex = n == 1 ? want32 : want8;
        CHECK(bhrt_sky_lookup(n == 1 ? s32 : s8, dirs, n, rgb) == 0, "lookup: %s", bhrt_last_error());
        for (int i = 0; i < 3 * n; i++) CHECK(rgb[i] == dirs[i] * 2.0 + 1.0, "lookup element %d", i);
        free(dirs);
        free(rgb);
    }
    g_want_tex = NULL;
    CHECK(g_sky_launches == 2, "sky launches %ld", g_sky_launches);
    /* refusals of a live object: no launch, nothing written, no HIP call but the query */
    g_hip = g_query = 0;
    CHECK(bhrt_sky_lookup(s32, NULL, 1, io + 3) == -1 && has("NULL"), "NULL dirs");
    CHECK(bhrt_sky_lookup(s32, io, 1, NULL) == -1 && has("NULL"), "NULL rgb");
    CHECK(bhrt_sky_lookup(s32, io, 0, io + 3) == -1 && has("n 0"), "n 0");
    CHECK(bhrt_sky_lookup_device(s32, io, -3, io + 3, NULL) == -1 && has("n -3"), "n -3");
    CHECK(g_hip == 0 && g_query == 0, "argument refusals made HIP calls");
    __real_hipSetDevice(1);
    CHECK(bhrt_sky_lookup(s32, io, 1, io + 3) == -1 && has("current device is 1"), "other device");
    CHECK(bhrt_sky_lookup_device(s32, io, 1, io + 3, NULL) == -1 && has("current device is 1"), "other device");
    __real_hipSetDevice(0);
    CHECK(g_hip == 0 && g_query == 2 && g_sky_launches == 2 && io[3] == 4 && io[5] == 6,
          "device refusals: %ld HIP calls, %ld queries", g_hip, g_query);

    /* ---- 3. frames ---- */
    int written = 0;
    CHECK(frame(0, 0, &written) == 0 && written && g_traces == 1 && !g_seen.tex && !g_seen.w &&
          !g_seen.chord, "the plain frame carries a sky block");
    long t0 = g_traces;
    CHECK(frame(BHRT_FLAG_SKY, 0, &written) == -1 && has("no sky map is bound") && !written &&
          g_traces == t0, "the flag without a map: %s", bhrt_last_error());
    CHECK(bhrt_set_sky(s32) == 0, "bind");
    CHECK(frame(0, 0, &written) == 0 && written && !g_seen.tex && !g_seen.w && g_seen_flags == 0,
          "a bound map without the flag reaches the launch");
    CHECK(frame(BHRT_FLAG_SKY | BHRT_FLAG_DOPPLER, 0, &written) == 0 && written && g_seen.tex &&
          g_seen.w == SW && g_seen.h == SH && g_seen.sx == SW / (2.0 * BH_PI) &&
          g_seen.sy == SH / BH_PI && g_seen.chord == NULL && g_seen_fused == 1 &&
          g_seen_flags == (BHRT_FLAG_SKY | BHRT_FLAG_DOPPLER), "the sky block of a fused frame");
    setenv("BHRT_FUSE_COLOUR", "0", 1);
    CHECK(frame(BHRT_FLAG_SKY, 1, &written) == 0 && g_seen.tex && g_seen.chord && g_seen_fused == 0,
          "the sky block of a frame with the separate pass: %s", bhrt_last_error());
    unsetenv("BHRT_FUSE_COLOUR");
    CHECK(bhrt_set_sky(s8) == 0 && frame(BHRT_FLAG_SKY, 0, NULL) == 0, "rebind");
    const void* tex8 = g_seen.tex;
    CHECK(bhrt_set_sky(s32) == 0 && frame(BHRT_FLAG_SKY, 0, NULL) == 0 && g_seen.tex != tex8, "rebind back");

    /* another device: the launch is refused before it is made */
    t0 = g_traces;
    __real_hipSetDevice(1);
    CHECK(frame(BHRT_FLAG_SKY, 0, &written) == -1 && has("lives on device 0") && !written && g_traces == t0,
          "a frame on device 1 with device 0's map: %s", bhrt_last_error());
    bhrt_sky* s1 = NULL;
    CHECK(bhrt_sky_create(f32, SW, SH, BHRT_SKY_RGB32F, &s1) == 0 && bhrt_sky_info(s1, &st) == 0 &&
          st.device == 1, "a map on device 1");
    CHECK(bhrt_set_sky(s1) == 0 && frame(BHRT_FLAG_SKY, 0, NULL) == 0 && g_traces == t0 + 1, "its frame");
    __real_hipSetDevice(0);
    t0 = g_traces;
    CHECK(frame(BHRT_FLAG_SKY, 0, &written) == -1 && has("lives on device 1") && !written && g_traces == t0,
          "a frame on device 0 with device 1's map");
    CHECK(bhrt_set_sky(s32) == 0, "bind");

    /* the multi-device splits: refused before any launch; one device passes */
    {
        enum { GW = 8, GH = 32 };
        uint8_t* host8 = (uint8_t*)malloc(4 * GW * GH);
        memset(host8, 0x77, 4 * GW * GH);
        bhrt_frame_soa out;
        memset(&out, 0, sizeof out);
        out.rgba8 = host8;
        t0 = g_traces;
        CHECK(bhrt_render_frame(&bh, &dk, &cfg, &cam, GW, GH, INTEGRATOR_RK4, BHRT_FLAG_SKY, &out) == -1 &&
              has("lives on device 0") && g_traces == t0 && host8[0] == 0x77, "host frame over 2 devices");
        CHECK(bhrt_render_frame(&bh, &dk, &cfg, &cam, GW, GH, INTEGRATOR_RK4, 0, &out) == 0 &&
              g_traces > t0, "the flagless host frame over 2 devices: %s", bhrt_last_error());
        setenv("BHRT_MAX_DEVICES", "1", 1);
        t0 = g_traces;
        CHECK(bhrt_render_frame(&bh, &dk, &cfg, &cam, GW, GH, INTEGRATOR_RK4, BHRT_FLAG_SKY, &out) == 0 &&
              g_traces > t0 && g_seen.tex, "host frame on one device: %s", bhrt_last_error());
        unsetenv("BHRT_MAX_DEVICES");
        void* d8 = NULL;
        if (__real_hipMalloc(&d8, 4 * GW * GH) != hipSuccess) abort();
        out.rgba8 = (uint8_t*)d8;
        t0 = g_traces;
        CHECK(bhrt_render_frame_gather(&bh, &dk, &cfg, &cam, GW, GH, INTEGRATOR_RK4, BHRT_FLAG_SKY, &out,
                                       2, 2, NULL) == -1 && has("lives on device 0") && g_traces == t0,
              "gather over 2 devices: %s", bhrt_last_error());
        CHECK(bhrt_render_frame_gather(&bh, &dk, &cfg, &cam, GW, GH, INTEGRATOR_RK4, BHRT_FLAG_SKY, &out,
                                       1, 1, NULL) == 0 && g_traces == t0 + 1, "gather on one device");
        __real_hipFree(d8);
        free(host8);
    }

    /* ---- 4. destroy: unbinds the bound map, frees the texels ---- */
    const void* tex = g_seen.tex;
    CHECK(fakehip_kind_of(tex, 16) == 0, "the bound map's texels");
    bhrt_sky_destroy(s8); /* not the bound one: s32 stays bound */
    CHECK(frame(BHRT_FLAG_SKY, 0, NULL) == 0 && g_seen.tex == tex, "destroy of another map unbound this one");
    bhrt_sky_destroy(s32);
    CHECK(fakehip_kind_of(tex, 16) != 0, "destroy left the texels allocated");
    t0 = g_traces;
    CHECK(frame(BHRT_FLAG_SKY, 0, &written) == -1 && has("no sky map is bound") && !written && g_traces == t0,
          "destroy did not unbind");
    CHECK(frame(0, 0, &written) == 0 && written, "the plain frame afterwards");
    __real_hipSetDevice(1);
    bhrt_sky_destroy(s1);
    __real_hipSetDevice(0);
    for (int i = 0; i < 50; i++) { /* create / destroy leaves nothing behind */
        bhrt_sky* s = NULL;
        CHECK(bhrt_sky_create(u8, SW, SH, BHRT_SKY_RGBA8, &s) == 0, "create %d", i);
        bhrt_sky_destroy(s);
    }
    free(f32);
    free(u8);
    free(want32);
    free(want8);
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld trace launches, %ld sky launches)\n", g_traces, g_sky_launches);
    return 0;
}
