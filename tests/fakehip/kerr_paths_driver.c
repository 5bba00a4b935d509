/* kerr_paths_driver.c -- physical photon paths (kerr_paths.c and kerr.c over the HOST_CORE files)
 * on SIMULATED devices (fake_hip.c), built by tests/test_kerr_paths_cpu.py under ASan+UBSan as a
 * stand-alone program.
 *
 * Both Kerr launchers are stubs: each checks that every buffer of its launch lies on the
 * simulated device, records the launch's parameters, its stream and its place in the order of
 * launches, and fills the outputs from host code -- the path launcher want_count(i) points per ray
 * whose coordinates encode (i, j, c), the k_kerr launcher an encoding of the ray id. The HIP entry
 * points the host code can reach are counted through the linker's --wrap, so "no HIP call" is
 * checked, not assumed.
 *
 * Checked: every refusal of include/bhrt_api.h "Physical photon paths" with zero HIP calls (the
 * current device's query aside, for the one refusal that needs it), nothing written and nothing
 * launched -- a bad device_hits leaves no path launch behind; what a launch carries (n,
 * max_positions, every, the three output pointers, the scene constants equal to
 * bhrt_kerr_rays_device's for the same scene); the hit launch queued after the path launch on the
 * same stream; the host form's three copy-back shapes with the elements beyond count untouched;
 * the statistics. Test infrastructure only. */
#include <limits.h>
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

static void on_device(const void* p, size_t n, const char* what) {
    if (!p) return;
    const int k = fakehip_kind_of(p, n);
    if (k != fakehip_current_device()) {
        fprintf(stderr, "launch buffer %s (%zu B) is memory kind %d, launching on device %d\n",
                what, n, k, fakehip_current_device());
        abort();
    }
}

/* ---- launcher stubs ---- */
static long g_seq;                      /* launches of either kind so far */
static long g_paths, g_paths_seq;       /* path launches; the last one's place in the order */
static long g_hits, g_hits_seq;         /* k_kerr launches */
static void *g_paths_stream, *g_hits_stream;
static bhrt_kparams g_pkp, g_hkp;
static bhrt_kerr_paths_k g_pk;
static bhrt_kerr_k g_kk;
static int g_full;                      /* every ray stores max_positions points */
static unsigned long long g_steps;      /* the steps the path launches reported */

static int want_count(int i, int P) { return g_full ? P : 1 + (i * 3 + 2) % P; }
static double enc(int i, int j, int c) { return i * 1000.0 + j * 4.0 + c + 0.5; }

int bhrt_launch_kerr_paths(const bhrt_kparams* kp, const bhrt_kerr_paths_k* pk, void* stream,
                           void* ev0, void* ev1) {
    (void)ev0; (void)ev1;
    const size_t n = (size_t)kp->n, P = (size_t)pk->max_positions;
    on_device(kp->rays, sizeof(Ray) * n, "rays");
    on_device(kp->ctl, 8 * 16, "control block");
    on_device(pk->out.xyz, sizeof(Vector3D) * n * P, "xyz");
    on_device(pk->out.xyz32, 12 * n * P, "xyz32");
    on_device(pk->out.count, 4 * n, "count");
    void* const* out = (void* const*)&kp->out;
    for (int f = 0; f < 15; f++)
        if (out[f]) {
            fprintf(stderr, "path launch with a hit field (the hits are k_kerr's launch)\n");
            abort();
        }
    if (kp->ctl[0] != 0) {
        fprintf(stderr, "claim counter not zero at launch\n");
        abort();
    }
    g_pkp = *kp;
    g_pk = *pk;
    for (size_t i = 0; i < n; i++) {
        const int cnt = want_count((int)i, (int)P);
        for (int j = 0; j < cnt; j++) {
            if (pk->out.xyz) {
                Vector3D* q = &pk->out.xyz[i * P + (size_t)j];
                q->x = enc((int)i, j, 0);
                q->y = enc((int)i, j, 1);
                q->z = enc((int)i, j, 2);
            }
            if (pk->out.xyz32)
                for (int c = 0; c < 3; c++)
                    pk->out.xyz32[(i * P + (size_t)j) * 3 + c] = (float)enc((int)i, j, c);
        }
        if (pk->out.count) pk->out.count[i] = cnt;
        kp->ctl[2] += (unsigned long long)(cnt - 1);
        g_steps += (unsigned long long)(cnt - 1);
    }
    kp->ctl[0] = (n + 63) / 64; /* (the kernel's claims) */
    kp->ctl[1] += n;
    g_paths++;
    g_paths_seq = ++g_seq;
    g_paths_stream = stream;
    return 0;
}

int bhrt_launch_kerr(const bhrt_kparams* kp, const bhrt_kerr_k* kk, void* stream, void* ev0,
                     void* ev1) {
    (void)ev0; (void)ev1;
    const size_t n = (size_t)kp->n;
    on_device(kp->ctl, 8 * 16, "control block");
    on_device(kp->rays, sizeof(Ray) * n, "rays");
    static const size_t fsize[15] = {4, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 16, 4};
    void* const* f = (void* const*)&kp->out;
    for (int i = 0; i < 15; i++) on_device(f[i], fsize[i] * n, "an output field");
    on_device(kk->h_residual, 8 * n, "h_residual");
    on_device(kk->lz_drift, 8 * n, "lz_drift");
    g_hkp = *kp;
    g_kk = *kk;
    for (size_t i = 0; i < n; i++) {
        if (kp->out.result) kp->out.result[i] = (int32_t)(i % 5);
        if (kp->out.hit_x) kp->out.hit_x[i] = (double)i + 0.25;
        if (kp->out.sky_x && i % 2 == 0) kp->out.sky_x[i] = -(double)i; /* (odd ones not written) */
        if (kp->out.rgb_r) kp->out.rgb_r[i] = kp->out.rgb_g[i] = kp->out.rgb_b[i] = 0.125;
        if (kk->h_residual) kk->h_residual[i] = 1e-6 * (double)i;
    }
    kp->ctl[1] += n;
    g_hits++;
    g_hits_seq = ++g_seq;
    g_hits_stream = stream;
    return 0;
}

int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)kp; (void)stream; (void)ev0; (void)ev1;
    fprintf(stderr, "a Kerr path call reached the parity trace launcher\n");
    abort();
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

static int has(const char* needle) { return strstr(bhrt_last_error(), needle) != NULL; }

static BlackHoleParams bh;
static AccretionDiskParams dk = {2.4, 12.0, 1.0, 1.0, 0.0, 0.0};
static SimulationConfig cfg;

#define SENT 777.0
#define SENT32 555.0f

/* one host-form call of n rays and P positions; which: bit 0 xyz, bit 1 xyz32, bit 2 count,
 * bit 3 hits (result, hit_x, sky_x), bit 4 diag */
static void run(int n, int P, int which, const char* what) {
    const size_t N = (size_t)n, np = N * (size_t)P;
    /* exact-size allocations: ASan sees one element too many */
    Ray* rays = (Ray*)malloc(N * sizeof(Ray));
    Vector3D* xyz = (Vector3D*)malloc(np * sizeof(Vector3D));
    float* xyz32 = (float*)malloc(np * 3 * sizeof(float));
    int32_t* count = (int32_t*)malloc(N * sizeof(int32_t));
    int32_t* result = (int32_t*)malloc(N * sizeof(int32_t));
    double* hx = (double*)malloc(N * sizeof(double));
    double* sx = (double*)malloc(N * sizeof(double));
    double* hres = (double*)malloc(N * sizeof(double));
    for (size_t i = 0; i < N; i++) {
        memset(&rays[i], 0, sizeof rays[i]);
        rays[i].origin.x = 20.0 + (double)i;
        rays[i].direction.y = 1.0;
        count[i] = -9;
        result[i] = -9;
        hx[i] = sx[i] = hres[i] = SENT;
    }
    for (size_t e = 0; e < np; e++) xyz[e].x = xyz[e].y = xyz[e].z = SENT;
    for (size_t e = 0; e < np * 3; e++) xyz32[e] = SENT32;
    bhrt_paths paths = {which & 1 ? xyz : NULL, which & 2 ? xyz32 : NULL, which & 4 ? count : NULL};
    bhrt_frame_soa hits;
    memset(&hits, 0, sizeof hits);
    hits.result = result;
    hits.hit_x = hx;
    hits.sky_x = sx;
    const bhrt_kerr_diag diag = {hres, NULL};
    const long before = g_paths, hits_before = g_hits;
    const int rc = bhrt_kerr_paths(rays, n, &bh, &dk, &cfg, P, 1, 0, &paths, which & 8 ? &hits : NULL,
                                   which & 16 ? &diag : NULL);
    CHECK(rc == 0, "%s: rc %d (%s)", what, rc, bhrt_last_error());
    CHECK(g_paths == before + 1, "%s: %ld path launches", what, g_paths - before);
    CHECK(g_hits == hits_before + (which & 8 ? 1 : 0), "%s: %ld hit launches", what,
          g_hits - hits_before);
    if (rc == 0) {
        CHECK(g_pkp.n == n && g_pk.max_positions == P && g_pk.every == 1, "%s: launch shape", what);
        CHECK(memcmp(g_pkp.rays, rays, N * sizeof(Ray)) == 0, "%s: the uploaded rays", what);
        if (which & 8)
            CHECK(g_hits_seq == g_paths_seq + 1 && g_hits_stream == g_paths_stream &&
                  g_hkp.rays == g_pkp.rays && g_hkp.n == n, "%s: the hit launch's order", what);
    }
    for (int i = 0; i < n && rc == 0; i++) {
        const int cnt = want_count(i, P);
        if (which & 4) CHECK(count[i] == cnt, "%s: count[%d] = %d, want %d", what, i, count[i], cnt);
        else CHECK(count[i] == -9, "%s: count[%d] written", what, i);
        for (int j = 0; j < P; j++) {
            const Vector3D q = xyz[(size_t)i * P + j];
            const float* q32 = &xyz32[((size_t)i * P + j) * 3];
            const int stored = j < cnt;
            if (which & 1 && stored)
                CHECK(q.x == enc(i, j, 0) && q.y == enc(i, j, 1) && q.z == enc(i, j, 2),
                      "%s: xyz[%d][%d] = %g %g %g", what, i, j, q.x, q.y, q.z);
            else
                CHECK(q.x == SENT && q.y == SENT && q.z == SENT,
                      "%s: xyz[%d][%d] beyond count %d was written: %g %g %g", what, i, j, cnt, q.x,
                      q.y, q.z);
            for (int c = 0; c < 3; c++)
                if (which & 2 && stored)
                    CHECK(q32[c] == (float)enc(i, j, c), "%s: xyz32[%d][%d][%d] = %g", what, i, j,
                          c, q32[c]);
                else
                    CHECK(q32[c] == SENT32, "%s: xyz32[%d][%d][%d] beyond count %d was written",
                          what, i, j, c, cnt);
        }
        if (which & 8)
            CHECK(result[i] == i % 5 && hx[i] == i + 0.25 && sx[i] == (i % 2 ? SENT : -(double)i),
                  "%s: hit record %d: %d %g %g", what, i, result[i], hx[i], sx[i]);
        else
            CHECK(result[i] == -9 && hx[i] == SENT && sx[i] == SENT, "%s: hit %d written", what, i);
        CHECK(hres[i] == (which & 16 ? 1e-6 * i : SENT), "%s: h_residual[%d] = %g", what, i, hres[i]);
    }
    free(rays);
    free(xyz);
    free(xyz32);
    free(count);
    free(result);
    free(hx);
    free(sx);
    free(hres);
}

int main(void) {
    initialize_black_hole_params(&bh, 1.0, 0.9, 0.0);
    memset(&cfg, 0, sizeof cfg);
    cfg.time_step = 0.25;
    cfg.max_ray_distance = 60.0;
    cfg.max_integration_steps = 2000;
    cfg.tolerance = 1e-6;
    enum { N = 130, P = 7 };

    /* poisoned host outputs: a refusal writes nothing */
    Ray* rays = (Ray*)malloc(sizeof(Ray) * N);
    Vector3D* xyz = (Vector3D*)malloc(sizeof(Vector3D) * N * P);
    float* xyz32 = (float*)malloc(12 * N * P);
    int32_t* count = (int32_t*)malloc(4 * N);
    int32_t* res = (int32_t*)malloc(4 * N);
    double* hx = (double*)malloc(8 * N);
    double* col = (double*)malloc(3 * 8 * N);
    double* dg = (double*)malloc(2 * 8 * N);
    for (int i = 0; i < N; i++) {
        memset(&rays[i], 0, sizeof rays[i]);
        rays[i].origin = (Vector3D){0.0, -18.0, 4.0};
        rays[i].direction = (Vector3D){0.0, 1.0, -0.2 + 1e-3 * i};
        count[i] = res[i] = -7;
        hx[i] = col[i] = col[N + i] = col[2 * N + i] = dg[i] = dg[N + i] = -7.0;
    }
    for (int e = 0; e < N * P; e++) {
        xyz[e].x = xyz[e].y = xyz[e].z = -7.0;
        xyz32[3 * e] = xyz32[3 * e + 1] = xyz32[3 * e + 2] = -7.0f;
    }
    const bhrt_paths paths = {xyz, xyz32, count};
    bhrt_frame_soa out;
    memset(&out, 0, sizeof out);
    out.result = res;
    out.hit_x = hx;
    out.rgb_r = col;
    out.rgb_g = col + N;
    out.rgb_b = col + 2 * N;
    const bhrt_kerr_diag diag = {dg, dg + N};

    /* ---- 1. refusals: zero HIP calls, not even the query; nothing written or launched ---- */
    g_hip = g_query = 0;
#define REFUSED(call, needle)                                                          \
    CHECK((call) == -1 && has(needle), "%s: rc or message: %s", #call, bhrt_last_error())
    /* both forms, with and without the hit records */
#define BOTH(R, NN, BH, DK, CFG, MP, EV, PA, HITS, DIAG, needle)                                    \
    do {                                                                                            \
        REFUSED(bhrt_kerr_paths_device(R, NN, BH, DK, CFG, MP, EV, 0, PA, HITS, DIAG, NULL), needle); \
        REFUSED(bhrt_kerr_paths(R, NN, BH, DK, CFG, MP, EV, 0, PA, HITS, DIAG), needle);            \
    } while (0)
#define SCENE(BH, DK, CFG, needle)                                              \
    do {                                                                        \
        BOTH(rays, N, BH, DK, CFG, P, 1, &paths, &out, &diag, needle);          \
        BOTH(rays, N, BH, DK, CFG, P, 1, &paths, NULL, NULL, needle);           \
    } while (0)
    SCENE(NULL, &dk, &cfg, "NULL");
    SCENE(&bh, &dk, NULL, "NULL");
    {
        const double spins[] = {1.0, -1.0, 1.5, NAN, INFINITY};
        for (int i = 0; i < 5; i++) {
            BlackHoleParams b = bh;
            b.spin = spins[i];
            SCENE(&b, &dk, &cfg, "spin");
        }
        const double masses[] = {0.0, -1.0, NAN, INFINITY};
        for (int i = 0; i < 4; i++) {
            BlackHoleParams b = bh;
            b.mass = masses[i];
            SCENE(&b, &dk, &cfg, "mass");
        }
        const double steps[] = {0.0, -0.25, NAN, INFINITY};
        for (int i = 0; i < 4; i++) {
            SimulationConfig c = cfg;
            c.time_step = steps[i];
            SCENE(&bh, &dk, &c, "time_step");
        }
        SimulationConfig c = cfg;
        c.max_integration_steps = -1;
        SCENE(&bh, &dk, &c, "max_integration_steps");
        c = cfg;
        c.max_ray_distance = NAN;
        SCENE(&bh, &dk, &c, "max_ray_distance");
        const double radii[][2] = {{NAN, 12.0}, {2.4, NAN}, {-1.0, 12.0}, {2.4, -12.0}};
        for (int i = 0; i < 4; i++) {
            AccretionDiskParams d = dk;
            d.inner_radius = radii[i][0];
            d.outer_radius = radii[i][1];
            SCENE(&bh, &d, &cfg, "disk radii");
        }
        /* a bad device_hits: refused with the path arguments, no path launch left behind */
        bhrt_frame_soa o = out;
        o.time_dilation = hx;
        BOTH(rays, N, &bh, &dk, &cfg, P, 1, &paths, &o, NULL, "time_dilation");
        o = out;
        o.rgb_g = NULL;
        BOTH(rays, N, &bh, &dk, &cfg, P, 1, &paths, &o, NULL, "rgb_r/g/b");
        o = out;
        o.rgb_r = o.rgb_g = NULL;
        BOTH(rays, N, &bh, &dk, &cfg, P, 1, &paths, &o, &diag, "rgb_r/g/b");
        CHECK(g_paths == 0 && g_hits == 0, "a bad device_hits left %ld + %ld launches", g_paths,
              g_hits);
    }
    BOTH(rays, 0, &bh, &dk, &cfg, P, 1, &paths, &out, NULL, "n = 0");
    BOTH(rays, -5, &bh, &dk, &cfg, P, 1, &paths, NULL, NULL, "n = -5");
    BOTH(NULL, N, &bh, &dk, &cfg, P, 1, &paths, &out, NULL, "rays must not be NULL");
    BOTH(rays, N, &bh, &dk, &cfg, 0, 1, &paths, &out, NULL, "max_positions = 0");
    BOTH(rays, N, &bh, &dk, &cfg, -3, 1, &paths, NULL, NULL, "max_positions = -3");
    BOTH(rays, N, &bh, &dk, &cfg, BHRT_PATHS_MAX_POSITIONS + 1, 1, &paths, NULL, NULL, "max_positions");
    BOTH(rays, N, &bh, &dk, &cfg, P, 0, &paths, &out, NULL, "every = 0");
    BOTH(rays, N, &bh, &dk, &cfg, P, -2, &paths, NULL, NULL, "every = -2");
    BOTH(rays, N, &bh, &dk, &cfg, P, 1, NULL, &out, NULL, "none of xyz, xyz32 and count");
    {
        const bhrt_paths none = {NULL, NULL, NULL};
        BOTH(rays, N, &bh, &dk, &cfg, P, 1, &none, NULL, NULL, "none of xyz, xyz32 and count");
    }
    /* (long)n * max_positions > INT_MAX: 32768 * 65536 = 2^31 (refused before a ray is read) */
    BOTH(rays, 32768, &bh, &dk, &cfg, BHRT_PATHS_MAX_POSITIONS, 1, &paths, NULL, NULL, "more than");
    BOTH(rays, INT_MAX, &bh, &dk, &cfg, 2, 1, &paths, &out, NULL, "more than");
    BOTH(rays, N, &bh, &dk, &cfg, P, 1, &paths, NULL, &diag, "hits is NULL");
    /* the host form alone: an origin without a static observer */
    {
        const Vector3D bad[] = {{0.5, 0.0, 0.0}, {1.0, 1.0, 0.0}, {1.9, 0.0, 0.0}, {NAN, 0.0, 0.0}};
        for (int i = 0; i < 4; i++) {
            const Vector3D keep = rays[N - 1].origin;
            rays[N - 1].origin = bad[i];
            REFUSED(bhrt_kerr_paths(rays, N, &bh, &dk, &cfg, P, 1, 0, &paths, &out, NULL), "of ray 129");
            REFUSED(bhrt_kerr_paths(rays, N, &bh, NULL, &cfg, P, 1, 0, &paths, NULL, NULL), "no static observer");
            rays[N - 1].origin = keep;
        }
    }
    CHECK(g_hip == 0 && g_query == 0, "refusals made %ld HIP calls, %ld queries", g_hip, g_query);
    /* the sky flag without a bound map: the current device's query and nothing else; without the
     * hit records the flag is not used, so that call is not refused for it (checked in 2.) */
    g_hip = g_query = 0;
    REFUSED(bhrt_kerr_paths_device(rays, N, &bh, &dk, &cfg, P, 1, BHRT_FLAG_SKY, &paths, &out, NULL, NULL),
            "no sky map is bound");
    REFUSED(bhrt_kerr_paths(rays, N, &bh, &dk, &cfg, P, 1, BHRT_FLAG_SKY, &paths, &out, NULL),
            "no sky map is bound");
    CHECK(g_hip == 0, "the sky refusal made %ld HIP calls", g_hip);
    for (int i = 0; i < N; i++)
        if (count[i] != -7 || res[i] != -7 || hx[i] != -7.0 || col[i] != -7.0 || dg[i] != -7.0 ||
            dg[N + i] != -7.0) {
            CHECK(0, "a refusal wrote element %d", i);
            break;
        }
    for (int e = 0; e < N * P; e++)
        if (xyz[e].x != -7.0 || xyz[e].z != -7.0 || xyz32[3 * e] != -7.0f || xyz32[3 * e + 2] != -7.0f) {
            CHECK(0, "a refusal wrote point %d", e);
            break;
        }
    CHECK(g_paths == 0 && g_hits == 0, "a refusal launched (%ld + %ld)", g_paths, g_hits);

    /* ---- 2. the device form: what the launches carry, and their order ---- */
    void *d_rays = NULL, *d_xyz = NULL, *d_xyz32 = NULL, *d_count = NULL, *d_res = NULL, *d_hx = NULL,
         *d_h = NULL;
    if (__real_hipMalloc(&d_rays, sizeof(Ray) * N) || __real_hipMalloc(&d_xyz, sizeof(Vector3D) * N * P) ||
        __real_hipMalloc(&d_xyz32, 12 * N * P) || __real_hipMalloc(&d_count, 4 * N) ||
        __real_hipMalloc(&d_res, 4 * N) || __real_hipMalloc(&d_hx, 8 * N) || __real_hipMalloc(&d_h, 8 * N))
        abort();
    memcpy(d_rays, rays, sizeof(Ray) * N);
    const bhrt_paths dpaths = {(Vector3D*)d_xyz, (float*)d_xyz32, (int32_t*)d_count};
    bhrt_frame_soa dout;
    memset(&dout, 0, sizeof dout);
    dout.result = (int32_t*)d_res;
    dout.hit_x = (double*)d_hx;
    const bhrt_kerr_diag ddiag = {(double*)d_h, NULL};
    /* paths alone (the unused sky flag is no refusal without the hit records) */
    CHECK(bhrt_kerr_paths_device((const Ray*)d_rays, N, &bh, &dk, &cfg, P, 3, BHRT_FLAG_SKY, &dpaths,
                                 NULL, NULL, NULL) == 0 && g_paths == 1 && g_hits == 0,
          "paths alone: %s", bhrt_last_error());
    CHECK(g_pkp.src == BHRT_SRC_RAYS && g_pkp.rays == (const Ray*)d_rays && g_pkp.n == N &&
          g_pk.max_positions == P && g_pk.every == 3 && g_pk.out.xyz == (Vector3D*)d_xyz &&
          g_pk.out.xyz32 == (float*)d_xyz32 && g_pk.out.count == (int32_t*)d_count, "the path launch");
    CHECK(g_pk.k.h_residual == NULL && g_pk.k.lz_drift == NULL, "diag pointers in a path launch");
    CHECK(((int32_t*)d_count)[5] == want_count(5, P) && ((Vector3D*)d_xyz)[5 * P].y == enc(5, 0, 1),
          "the path launch's outputs");
    /* with the hit records: k_kerr's launch behind it, on the same stream, the same constants */
    CHECK(bhrt_kerr_paths_device((const Ray*)d_rays, N - 3, &bh, &dk, &cfg, P, 1, BHRT_FLAG_DOPPLER,
                                 &dpaths, &dout, &ddiag, NULL) == 0 && g_paths == 2 && g_hits == 1,
          "paths and hits: %s", bhrt_last_error());
    CHECK(g_hits_seq == g_paths_seq + 1 && g_hits_stream == g_paths_stream && g_hits_stream != NULL,
          "order: path launch %ld, hit launch %ld, streams %p %p", g_paths_seq, g_hits_seq,
          g_paths_stream, g_hits_stream);
    CHECK(g_hkp.src == BHRT_SRC_RAYS && g_hkp.rays == (const Ray*)d_rays && g_hkp.n == N - 3 &&
          g_pkp.n == N - 3 && g_hkp.sc.flags == BHRT_FLAG_DOPPLER && g_hkp.out.result == (int32_t*)d_res &&
          g_kk.h_residual == (double*)d_h && g_kk.lz_drift == NULL, "the hit launch");
    const bhrt_kerr_k via_paths = g_kk, in_paths = g_pk.k;
    /* ... equal to what bhrt_kerr_rays_device launches for the same scene */
    CHECK(bhrt_kerr_rays_device((const Ray*)d_rays, N - 3, &bh, &dk, &cfg, BHRT_FLAG_DOPPLER, &dout,
                                &ddiag, NULL) == 0 && g_hits == 2, "rays: %s", bhrt_last_error());
    CHECK(memcmp(&via_paths, &g_kk, sizeof g_kk) == 0, "the hit launch's constants");
#define SAME(field) CHECK(in_paths.field == g_kk.field, "the path launch's " #field)
    SAME(M); SAME(two_m); SAME(a); SAME(a2); SAME(r_plus); SAME(eight_m); SAME(dt); SAME(max_dist);
    SAME(disk_lo); SAME(disk_hi); SAME(max_steps); SAME(has_disk);
    CHECK(in_paths.a == -0.9 && in_paths.r_plus == 1.0 + sqrt(1.0 - 0.9 * 0.9) && in_paths.dt == 0.25 &&
          in_paths.max_steps == 2000 && in_paths.has_disk == 1 &&
          in_paths.disk_lo == 2.4 * 2.4 + 0.9 * 0.9, "the scene constants");
    /* an explicit stream is used as given, by both launches */
    {
        hipStream_t s = NULL;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess || !s) abort();
        SimulationConfig c = cfg; /* zero steps and no disk are scenes, not refusals */
        c.max_integration_steps = 0;
        CHECK(bhrt_kerr_paths_device((const Ray*)d_rays, 1, &bh, NULL, &c, 1, 100000, 0, &dpaths,
                                     &dout, NULL, (void*)s) == 0 && g_paths_stream == (void*)s &&
              g_hits_stream == (void*)s && g_hits_seq == g_paths_seq + 1 && g_pk.k.max_steps == 0 &&
              g_pk.k.has_disk == 0 && g_pk.every == 100000 && g_pkp.n == 1,
              "explicit stream: %s", bhrt_last_error());
    }
    /* the statistics: path launches count as trace launches, and so do the hit launches */
    {
        bhrt_stats st;
        CHECK(bhrt_get_stats(&st, 1) == 0 && st.launches == (uint64_t)(g_paths + g_hits) &&
              st.rays == (uint64_t)(N + 3 * (N - 3) + 2) && st.iterations == g_steps,
              "stats: %llu launches, %llu rays, %llu iterations (%llu steps reported)",
              (unsigned long long)st.launches, (unsigned long long)st.rays,
              (unsigned long long)st.iterations, g_steps);
    }

    /* ---- 3. the host form: the three copy-back shapes; tails untouched ---- */
    static const int combos[] = {1 | 4 | 8, 2 | 4, 1, 2 | 8 | 16, 4, 1 | 2 | 4 | 8 | 16};
    char what[96];
    /* readback forms (host_frames.c bhrt_rows_back): the staged rectangle (the default for rows
     * this short), one copy per ray (a copy call priced at 0 bytes), one rectangle (every row
     * full) */
    for (int form = 0; form < 3; form++) {
        if (form == 1) setenv("BHRT_PATHS_COPY_CALL_BYTES", "0", 1);
        else unsetenv("BHRT_PATHS_COPY_CALL_BYTES");
        g_full = form == 2;
        for (int k = 0; k < (int)(sizeof combos / sizeof *combos); k++)
            for (int n = 1; n <= 5; n += 4)
                for (int p = 1; p <= 7; p += 3) {
                    snprintf(what, sizeof what, "form %d outputs %d n %d P %d", form, combos[k], n, p);
                    run(n, p, combos[k], what);
                }
    }
    g_full = 0;
    __real_hipFree(d_rays);
    __real_hipFree(d_xyz);
    __real_hipFree(d_xyz32);
    __real_hipFree(d_count);
    __real_hipFree(d_res);
    __real_hipFree(d_hx);
    __real_hipFree(d_h);
    free(rays);
    free(xyz);
    free(xyz32);
    free(count);
    free(res);
    free(hx);
    free(col);
    free(dg);
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld path launches, %ld hit launches)\n", g_paths, g_hits);
    return 0;
}
