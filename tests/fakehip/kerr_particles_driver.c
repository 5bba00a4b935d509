/* kerr_particles_driver.c -- the host side of the physical particle update (kerr_particles.c on
 * the resident object of particles_resident.c, with kerr.c, whose scene checks it shares, over the
 * HOST_CORE files) on SIMULATED devices (fake_hip.c), built by tests/test_kerr_particles_cpu.py
 * under ASan+UBSan as a stand-alone program.
 *
 * The new launcher is a stub that checks its buffers against the simulated device and records what
 * the launch carries. The HIP entry points the host code can reach are counted through the
 * linker's --wrap, so "no HIP call" is checked, not assumed.
 *
 * Checked: every refusal of include/bhrt_api.h "Physical particles" with zero HIP calls, no launch
 * and `updates` unchanged; steps == 0 launches nothing; a good call makes one launch with the
 * object's array, count and block counts, the call's steps, constants, diagnostics and stream;
 * `updates` advances at the call; the waiting calls wait for the update's stream; an object is
 * refused on a second device. Test infrastructure only. */
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

/* ---- HIP calls, counted (-Wl,--wrap=...) ---- */
static long g_hip;
static hipStream_t g_synced; /* the stream of the last hipStreamSynchronize */
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
WRAP(hipError_t, hipEventRecord, (hipEvent_t e, hipStream_t s), (e, s))
WRAP(hipError_t, hipStreamWaitEvent, (hipStream_t s, hipEvent_t e, unsigned f), (s, e, f))
WRAP(hipError_t, hipHostMalloc, (void** p, size_t n, unsigned f), (p, n, f))
hipError_t __real_hipStreamSynchronize(hipStream_t s);
hipError_t __wrap_hipStreamSynchronize(hipStream_t s) {
    g_hip++;
    g_synced = s;
    return __real_hipStreamSynchronize(s);
}
hipError_t __real_hipGetDevice(int* d); /* the current device's query: allowed before a refusal */
hipError_t __wrap_hipGetDevice(int* d) { return __real_hipGetDevice(d); }

static void on_device(const void* p, size_t n, const char* what) {
    if (!p) DIE("launch buffer %s is NULL", what);
    const int k = fakehip_kind_of(p, n);
    if (k != fakehip_current_device())
        DIE("launch buffer %s (%zu B) is memory kind %d, launching on device %d", what, n, k,
            fakehip_current_device());
}

static int nblocks_of(int count) { return (count + 255) / 256; }

/* ---- the launcher under test: a stub that records the launch ---- */
static long g_launches;
static struct {
    Particle* d;
    int count, steps;
    bhrt_kerr_particles_k k;
    int* blocks;
    void* stream;
} g_last;

int bhrt_launch_kerr_particles(Particle* d, int count, const bhrt_kerr_particles_k* k, int steps,
                               int* d_block_active, void* stream, void* ev0, void* ev1) {
    (void)ev0; (void)ev1;
    on_device(d, (size_t)count * sizeof(Particle), "particles");
    on_device(d_block_active, (size_t)nblocks_of(count) * sizeof(int), "block_active");
    if (k->k.h_residual) on_device(k->k.h_residual, 8 * (size_t)count, "h_residual");
    if (k->k.lz_drift) on_device(k->k.lz_drift, 8 * (size_t)count, "lz_drift");
    if (k->status) on_device(k->status, 4 * (size_t)count, "status");
    if (k->substeps_out) on_device(k->substeps_out, 4 * (size_t)count, "substeps");
    g_last.d = d;
    g_last.count = count;
    g_last.steps = steps;
    g_last.k = *k;
    g_last.blocks = d_block_active;
    g_last.stream = stream;
    g_launches++;
    return 0;
}

/* ---- the launchers the other linked files name ---- */
int bhrt_launch_particles_count(const Particle* d, int count, int* block_active, void* stream) {
    (void)stream;
    on_device(d, (size_t)count * sizeof(Particle), "particles");
    on_device(block_active, (size_t)nblocks_of(count) * sizeof(int), "block_active");
    for (int b = 0; b < nblocks_of(count); b++) {
        int c = 0;
        for (int i = 256 * b; i < count && i < 256 * (b + 1); i++) c += d[i].active != 0;
        block_active[b] = c;
    }
    return 0;
}
#define UNREACHED(name) DIE("a physical particle call reached " name)
int bhrt_launch_particles_counted(Particle* d, int count, const bhrt_particle_k* k, int steps,
                                  int* b, void* stream, void* ev0, void* ev1) {
    (void)d; (void)count; (void)k; (void)steps; (void)b; (void)stream; (void)ev0; (void)ev1;
    UNREACHED("the parity update");
}
int bhrt_launch_particles_scan(const int* b, int nb, int* o, void* stream, void* ev0, void* ev1) {
    (void)b; (void)nb; (void)o; (void)stream; (void)ev0; (void)ev1;
    UNREACHED("the scan");
}
int bhrt_launch_particles_scatter(const Particle* d, int count, const int* o, int m,
                                  const bhrt_particle_data* out, void* stream, void* ev0,
                                  void* ev1) {
    (void)d; (void)count; (void)o; (void)m; (void)out; (void)stream; (void)ev0; (void)ev1;
    UNREACHED("the scatter");
}
int bhrt_launch_particles(Particle* d, int count, const bhrt_particle_k* k, int steps,
                          void* stream, void* ev0, void* ev1) {
    (void)d; (void)count; (void)k; (void)steps; (void)stream; (void)ev0; (void)ev1;
    UNREACHED("the host particle update");
}
int bhrt_launch_kerr(const bhrt_kparams* kp, const bhrt_kerr_k* kk, void* stream, void* ev0,
                     void* ev1) {
    (void)kp; (void)kk; (void)stream; (void)ev0; (void)ev1;
    UNREACHED("the ray launcher");
}
int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)kp; (void)stream; (void)ev0; (void)ev1;
    UNREACHED("the parity trace launcher");
}
int bhrt_launch_path(const bhrt_kparams* kp, const double* o, const double* d, Vector3D* p,
                     int m, int* nn, int nin, void* st) {
    (void)kp; (void)o; (void)d; (void)p; (void)m; (void)nn; (void)nin; (void)st;
    UNREACHED("the path launcher");
}
hipError_t hipEventDestroy(hipEvent_t e) { /* (fake_hip.c has none) */
    free(e);
    return hipSuccess;
}

static BlackHoleParams g_bh;
static SimulationConfig g_cfg;

static int64_t updates_of(bhrt_particles* ps) {
    bhrt_particles_state st;
    if (bhrt_particles_info(ps, &st) != 0) DIE("info: %s", bhrt_last_error());
    return st.updates;
}

/* one refused call: -1, a message naming `word`, no HIP call, no launch, updates as they were */
static int g_refused;
static void refused(const char* what, const char* word, bhrt_particles* live, bhrt_particles* ps,
                    const BlackHoleParams* bh, const SimulationConfig* cfg, int steps,
                    const bhrt_kerr_particles_params* par, const bhrt_kerr_particles_diag* dg,
                    hipStream_t st) {
    const long hip0 = g_hip, l0 = g_launches;
    const int64_t u0 = updates_of(live);
    const int rc = bhrt_particles_kerr_update_device(ps, bh, cfg, steps, par, dg, st);
    CHECK(rc == -1, "%s: rc %d", what, rc);
    CHECK(strstr(bhrt_last_error(), word) != NULL, "%s: message '%s'", what, bhrt_last_error());
    CHECK(g_hip == hip0, "%s: %ld HIP calls before the refusal", what, g_hip - hip0);
    CHECK(g_launches == l0, "%s: launched", what);
    CHECK(updates_of(live) == u0, "%s: updates moved", what);
    g_refused++;
}

int main(void) {
    initialize_black_hole_params(&g_bh, 1.0, 0.9, 0.0);
    memset(&g_cfg, 0, sizeof g_cfg);
    g_cfg.time_step = 0.5;
    g_cfg.max_integration_steps = -5; /* of the config the time step alone is read */
    g_cfg.max_ray_distance = NAN;
    const int n = 300;
    ParticleSystem sys;
    if (particle_system_init(&sys, n) != 0) DIE("particle_system_init");
    for (int i = 0; i < n; i++) {
        const Vector3D x = {6.0 + i, 0.0, 0.0}, v = {0.0, 0.1, 0.0};
        if (add_particle(&sys, &x, &v, 1.0, (ParticleType)(i % 4)) < 0) DIE("add_particle");
        if (i % 3 == 0) sys.particles[i].active = 0;
    }
    hipStream_t st;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) DIE("stream");
    bhrt_particles* ps = NULL;
    if (bhrt_particles_create(&sys, &ps) != 0) DIE("create: %s", bhrt_last_error());
    const Particle* d_buf = NULL;
    (void)bhrt_particles_device_buffer(ps, &d_buf, NULL);
    double* d_f64 = NULL;
    int* d_i32 = NULL;
    if (hipMalloc((void**)&d_f64, 16 * (size_t)n) != hipSuccess ||
        hipMalloc((void**)&d_i32, 8 * (size_t)n) != hipSuccess)
        DIE("hipMalloc");
    const bhrt_kerr_particles_diag dg = {d_f64, d_f64 + n, d_i32, d_i32 + n};
    const bhrt_kerr_particles_params par = {2};

    /* ---- the refusals ---- */
    BlackHoleParams b = g_bh;
    SimulationConfig c = g_cfg;
    bhrt_kerr_particles_params bad = par;
    refused("NULL object", "NULL object", ps, NULL, &g_bh, &g_cfg, 1, &par, &dg, st);
    refused("NULL blackhole", "NULL", ps, ps, NULL, &g_cfg, 1, &par, &dg, st);
    refused("NULL config", "NULL", ps, ps, &g_bh, NULL, 1, &par, &dg, st);
    refused("steps -1", "steps", ps, ps, &g_bh, &g_cfg, -1, &par, &dg, st);
    b.spin = 1.0;
    refused("spin 1", "spin", ps, ps, &b, &g_cfg, 1, &par, &dg, st);
    b.spin = -1.5;
    refused("spin -1.5", "spin", ps, ps, &b, &g_cfg, 1, &par, &dg, st);
    b.spin = NAN;
    refused("spin NaN", "spin", ps, ps, &b, &g_cfg, 1, &par, &dg, st);
    b = g_bh;
    b.mass = 0.0;
    refused("mass 0", "mass", ps, ps, &b, &g_cfg, 1, &par, &dg, st);
    b.mass = INFINITY;
    refused("mass inf", "mass", ps, ps, &b, &g_cfg, 1, &par, &dg, st);
    b.mass = NAN;
    refused("mass NaN", "mass", ps, ps, &b, &g_cfg, 1, &par, &dg, st);
    c.time_step = 0.0;
    refused("time_step 0", "time_step", ps, ps, &g_bh, &c, 1, &par, &dg, st);
    c.time_step = NAN;
    refused("time_step NaN", "time_step", ps, ps, &g_bh, &c, 1, &par, &dg, st);
    c.time_step = INFINITY;
    refused("time_step inf", "time_step", ps, ps, &g_bh, &c, 1, &par, &dg, st);
    refused("NULL params", "params", ps, ps, &g_bh, &g_cfg, 1, NULL, &dg, st);
    bad.substeps = 0;
    refused("substeps 0", "substeps", ps, ps, &g_bh, &g_cfg, 1, &bad, &dg, st);
    bad.substeps = 65;
    refused("substeps 65", "substeps", ps, ps, &g_bh, &g_cfg, 1, &bad, &dg, st);
    bad.substeps = -1;
    refused("substeps -1", "substeps", ps, ps, &g_bh, &g_cfg, 0, &bad, NULL, NULL);
    /* a refusal is a refusal with steps == 0 too */
    refused("NULL params, steps 0", "params", ps, ps, &g_bh, &g_cfg, 0, NULL, NULL, st);

    /* ---- steps == 0: a no-op ---- */
    long hip0 = g_hip, l0 = g_launches;
    CHECK(bhrt_particles_kerr_update_device(ps, &g_bh, &g_cfg, 0, &par, &dg, st) == 0, "steps 0: %s",
          bhrt_last_error());
    CHECK(g_launches == l0 && g_hip == hip0 && updates_of(ps) == 0, "steps 0 did something");

    /* ---- a good call on a stream ---- */
    CHECK(bhrt_particles_kerr_update_device(ps, &g_bh, &g_cfg, 7, &par, &dg, st) == 0, "update: %s",
          bhrt_last_error());
    CHECK(g_launches == l0 + 1, "%ld launches", g_launches - l0);
    CHECK(g_last.d == d_buf && g_last.count == n && g_last.steps == 7, "array, count or steps");
    CHECK(g_last.stream == (void*)st, "the launch is not on the caller's stream");
    const bhrt_kerr_k* k = &g_last.k.k;
    CHECK(k->a == g_bh.spin * g_bh.mass && k->a2 == k->a * k->a && k->M == g_bh.mass &&
              k->two_m == 2.0 * g_bh.mass && k->eight_m == 8.0 * g_bh.mass &&
              k->dt == g_cfg.time_step &&
              k->r_plus == g_bh.mass + sqrt(g_bh.mass * g_bh.mass - k->a2),
          "the launch's constants (a = %g)", k->a);
    CHECK(g_last.k.substeps == 2 && k->h_residual == dg.h_residual && k->lz_drift == dg.lz_drift &&
              g_last.k.status == dg.status && g_last.k.substeps_out == dg.substeps,
          "substeps or the diagnostics' planes");
    CHECK(updates_of(ps) == 1, "updates after one call: %lld", (long long)updates_of(ps));
    /* the waiting calls wait for the update's stream */
    ParticleSystem back;
    if (particle_system_init(&back, n) != 0) DIE("particle_system_init");
    back.count = n;
    g_synced = NULL;
    CHECK(bhrt_particles_download(ps, &back) == 0, "download: %s", bhrt_last_error());
    CHECK(g_synced == st, "download did not wait for the update's stream");
    CHECK(memcmp(back.particles, sys.particles, (size_t)n * sizeof(Particle)) == 0,
          "the stub moved nothing, the download differs");

    /* ---- NULL stream, no diagnostics ---- */
    CHECK(bhrt_particles_kerr_update_device(ps, &g_bh, &g_cfg, 1, &par, NULL, NULL) == 0,
          "NULL stream: %s", bhrt_last_error());
    CHECK(g_launches == l0 + 2 && g_last.stream != NULL && g_last.stream != (void*)st,
          "NULL stream: the launch runs on the library's own stream");
    CHECK(!g_last.k.k.h_residual && !g_last.k.k.lz_drift && !g_last.k.status &&
              !g_last.k.substeps_out, "NULL diag left a plane set");
    CHECK(updates_of(ps) == 2, "updates after two calls");
    g_synced = NULL;
    CHECK(bhrt_particles_upload(ps, &sys) == 0, "upload: %s", bhrt_last_error());
    CHECK(g_synced == (hipStream_t)g_last.stream, "upload did not wait for the update's stream");

    /* ---- an object is bound to its device ---- */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 1) {
        if (hipSetDevice(1) != hipSuccess) DIE("hipSetDevice(1)");
        hipStream_t st1;
        if (hipStreamCreateWithFlags(&st1, hipStreamNonBlocking) != hipSuccess) DIE("stream");
        refused("another device", "current device", ps, ps, &g_bh, &g_cfg, 1, &par, NULL, st1);
        if (hipSetDevice(0) != hipSuccess) DIE("hipSetDevice(0)");
    } else {
        CHECK(0, "the driver needs two simulated devices (FAKEHIP_DEVICES=2)");
    }
    bhrt_particles_destroy(ps);
    (void)hipFree(d_f64);
    (void)hipFree(d_i32);
    particle_system_cleanup(&sys);
    particle_system_cleanup(&back);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%d refusals with no HIP call, %ld launches)\n", g_refused,
           g_launches);
    return 0;
}
