/* kerr_emit_driver.c -- Kerr disk emission (kerr_emit.c and kerr.c, whose checks it shares, over
 * the HOST_CORE files) on SIMULATED devices (fake_hip.c), built by tests/test_kerr_emit_cpu.py
 * under ASan+UBSan as a stand-alone program.
 *
 * The emission launcher is a stub: it checks that every buffer of the launch lies on the simulated
 * device, records the launch's parameters and fills the outputs with an encoding of the ray id;
 * the fixed-step launcher aborts, for no emission call may reach it. The HIP entry points the host
 * code can reach are counted through the linker's --wrap, so "no HIP call" is checked, not assumed.
 *
 * Checked: every refusal of include/bhrt_api.h "Kerr disk emission" -- those of the adaptive calls
 * and the emission's own -- with zero HIP calls and nothing written, counted and printed; what a
 * launch carries (K, q, gain, the physical spin, the tolerance, the output planes); the host forms'
 * round trips with radius / redshift elements kept where the kernel does not write them; the
 * statistics; bhrt_kerr_disk_redshift. Test infrastructure only. */
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
    const int k = fakehip_kind_of(p, n);
    if (k != fakehip_current_device()) {
        fprintf(stderr, "launch buffer %s (%zu B) is memory kind %d, launching on device %d\n",
                what, n, k, fakehip_current_device());
        abort();
    }
}

/* ---- launcher stubs ---- */
static long g_launches;
static bhrt_kparams g_kp;
static bhrt_kerr_emit_k g_ek;

int bhrt_launch_kerr(const bhrt_kparams* kp, const bhrt_kerr_k* kk, void* stream, void* ev0,
                     void* ev1) {
    (void)kp; (void)kk; (void)stream; (void)ev0; (void)ev1;
    fprintf(stderr, "an emission call reached the fixed-step launcher\n");
    abort();
}

/* ray i has i % (K + 1) crossings: plane k holds i + k / 8 (radius) and -(i + k / 8) (redshift)
 * below its count, and is left alone at and above it */
int bhrt_launch_kerr_emit(const bhrt_kparams* kp, const bhrt_kerr_emit_k* ek, void* stream,
                          void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    const bhrt_kerr_k* kk = &ek->rk.k;
    const size_t n = (size_t)kp->n, K = (size_t)ek->max_crossings;
    on_device(kp->ctl, 8 * 16, "control block");
    if (kp->src == BHRT_SRC_RAYS) on_device(kp->rays, sizeof(Ray) * n, "rays");
    static const size_t fsize[15] = {4, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 16, 4};
    void* const* f = (void* const*)&kp->out;
    for (int i = 0; i < 15; i++)
        if (f[i]) on_device(f[i], fsize[i] * n, "an output field");
    if (kk->h_residual) on_device(kk->h_residual, 8 * n, "h_residual");
    if (kk->lz_drift) on_device(kk->lz_drift, 8 * n, "lz_drift");
    if (ek->rk.rejected) on_device(ek->rk.rejected, 4 * n, "rejected");
    if (ek->out.count) on_device(ek->out.count, 4 * n, "count");
    if (ek->out.radius) on_device(ek->out.radius, 8 * K * n, "radius");
    if (ek->out.redshift) on_device(ek->out.redshift, 8 * K * n, "redshift");
    if (ek->out.intensity) on_device(ek->out.intensity, 8 * n, "intensity");
    g_kp = *kp;
    g_ek = *ek;
    for (size_t i = 0; i < n; i++) {
        const size_t cnt = i % (K + 1);
        if (kp->out.result) kp->out.result[i] = (int32_t)(i % 5);
        if (kp->out.steps) kp->out.steps[i] = (int32_t)i;
        if (kp->out.hit_x) kp->out.hit_x[i] = (double)i + 0.25;
        if (kp->out.sky_x && i % 2 == 0) kp->out.sky_x[i] = -(double)i; /* (odd ones not written) */
        if (kp->out.rgb_r) kp->out.rgb_r[i] = kp->out.rgb_g[i] = kp->out.rgb_b[i] = 0.125;
        if (kk->h_residual) kk->h_residual[i] = 1e-6 * (double)i;
        if (ek->rk.rejected) ek->rk.rejected[i] = (int)(i % 3);
        if (ek->out.count) ek->out.count[i] = (int)cnt;
        if (ek->out.intensity) ek->out.intensity[i] = 0.5 * (double)i;
        for (size_t k = 0; k < cnt; k++) {
            if (ek->out.radius) ek->out.radius[k * n + i] = (double)i + (double)k / 8.0;
            if (ek->out.redshift) ek->out.redshift[k * n + i] = -((double)i + (double)k / 8.0);
        }
    }
    kp->ctl[1] += n;
    kp->ctl[2] += 3 * n;
    g_launches++;
    return 0;
}

int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)kp; (void)stream; (void)ev0; (void)ev1;
    fprintf(stderr, "an emission call reached the parity trace launcher\n");
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

static long g_refusals; /* refusals checked (printed: the CPU test pins the count) */
static int has(const char* needle) { return strstr(bhrt_last_error(), needle) != NULL; }

static BlackHoleParams bh;
static AccretionDiskParams dk = {2.4, 12.0, 1.0, 1.0, 0.0, 0.0};
static SimulationConfig cfg;
static bhrt_camera cam = {{0.0, -18.0, 4.0}, {0.0, 18.0, -4.0}, {0.0, 0.0, 1.0}, 40.0, 0, 0.0, 0.0};

int main(void) {
    initialize_black_hole_params(&bh, 1.0, 0.9, 0.0);
    memset(&cfg, 0, sizeof cfg);
    cfg.time_step = 0.25;
    cfg.max_ray_distance = 60.0;
    cfg.max_integration_steps = 2000;
    cfg.tolerance = 1e-8;
    enum { W = 49, H = 27, N = W * H, K = 3 };
    const bhrt_kerr_emit_params ep = {K, 3.0, 1.5};

    /* poisoned host outputs: a refusal writes nothing */
    int32_t* res = (int32_t*)malloc(4 * N);
    double* hx = (double*)malloc(8 * N);
    double* sx = (double*)malloc(8 * N);
    double* col = (double*)malloc(3 * 8 * N);
    double* dg = (double*)malloc(8 * N);
    int* rj = (int*)malloc(4 * N);
    int* cnt = (int*)malloc(4 * N);
    double* rad = (double*)malloc(8 * K * N);
    double* red = (double*)malloc(8 * K * N);
    double* inten = (double*)malloc(8 * N);
    Ray* rays = (Ray*)malloc(sizeof(Ray) * N);
    for (int i = 0; i < N; i++) {
        res[i] = cnt[i] = rj[i] = -7;
        hx[i] = sx[i] = dg[i] = inten[i] = -7.0;
        col[i] = col[N + i] = col[2 * N + i] = -7.0;
        for (int k = 0; k < K; k++) rad[k * N + i] = red[k * N + i] = -7.0;
        rays[i].origin = cam.position;
        rays[i].direction = (Vector3D){0.0, 1.0, -0.2 + 1e-3 * i};
    }
    bhrt_frame_soa out;
    memset(&out, 0, sizeof out);
    out.result = res;
    out.hit_x = hx;
    out.sky_x = sx;
    out.rgb_r = col;
    out.rgb_g = col + N;
    out.rgb_b = col + 2 * N;
    const bhrt_kerr_rk45_diag diag = {dg, NULL, rj};
    const bhrt_kerr_emit_out eo = {cnt, rad, red, inten};

    /* ---- 1. refusals: zero HIP calls, not even the query; nothing written ---- */
    g_hip = g_query = 0;
#define REFUSED(call, needle)                                                          \
    do {                                                                               \
        g_refusals++;                                                                  \
        CHECK((call) == -1 && has(needle), "%s: rc or message: %s", #call, bhrt_last_error()); \
    } while (0)
#define ALL4F(BH, DK, CFG, FL, OUT, EP, EO, needle)                                               \
    do {                                                                                          \
        REFUSED(bhrt_kerr_emit_frame_device(BH, DK, CFG, &cam, W, H, NULL, FL, OUT, &diag, EP, EO, NULL), needle); \
        REFUSED(bhrt_kerr_emit_frame(BH, DK, CFG, &cam, W, H, FL, OUT, &diag, EP, EO), needle);   \
        REFUSED(bhrt_kerr_emit_rays_device(rays, N, BH, DK, CFG, FL, OUT, &diag, EP, EO, NULL), needle); \
        REFUSED(bhrt_kerr_emit_rays(rays, N, BH, DK, CFG, FL, OUT, &diag, EP, EO), needle);       \
    } while (0)
#define ALL4(BH, DK, CFG, OUT, needle) ALL4F(BH, DK, CFG, 0, OUT, &ep, &eo, needle)
    /* everything the adaptive calls refuse */
    ALL4(NULL, &dk, &cfg, &out, "NULL");
    ALL4(&bh, &dk, NULL, &out, "NULL");
    ALL4(&bh, &dk, &cfg, NULL, "NULL");
    {
        const double spins[] = {1.0, -1.0, 1.5, NAN, INFINITY};
        for (int i = 0; i < 5; i++) {
            BlackHoleParams b = bh;
            b.spin = spins[i];
            ALL4(&b, &dk, &cfg, &out, "spin");
        }
        const double masses[] = {0.0, -1.0, NAN, INFINITY};
        for (int i = 0; i < 4; i++) {
            BlackHoleParams b = bh;
            b.mass = masses[i];
            ALL4(&b, &dk, &cfg, &out, "mass");
        }
        const double steps[] = {0.0, -0.25, NAN, INFINITY};
        for (int i = 0; i < 4; i++) {
            SimulationConfig c = cfg;
            c.time_step = steps[i];
            ALL4(&bh, &dk, &c, &out, "time_step");
        }
        const double tols[] = {0.0, -1e-8, 9.99e-13, 1.0000001e-2, 1.0, NAN, INFINITY, -INFINITY};
        for (int i = 0; i < 8; i++) {
            SimulationConfig c = cfg;
            c.tolerance = tols[i];
            ALL4(&bh, &dk, &c, &out, "tolerance");
        }
        SimulationConfig c = cfg;
        c.max_integration_steps = -1;
        ALL4(&bh, &dk, &c, &out, "max_integration_steps");
        c = cfg;
        c.max_ray_distance = NAN;
        ALL4(&bh, &dk, &c, &out, "max_ray_distance");
        const double radii[][2] = {{NAN, 12.0}, {2.4, NAN}, {-1.0, 12.0}, {2.4, -12.0}};
        for (int i = 0; i < 4; i++) {
            AccretionDiskParams d = dk;
            d.inner_radius = radii[i][0];
            d.outer_radius = radii[i][1];
            ALL4(&bh, &d, &cfg, &out, "disk radii");
        }
        bhrt_frame_soa o = out;
        o.time_dilation = hx;
        ALL4(&bh, &dk, &cfg, &o, "time_dilation");
        o = out;
        o.rgb_g = NULL;
        ALL4(&bh, &dk, &cfg, &o, "rgb_r/g/b");
    }
    /* the emission's own */
    ALL4(&bh, NULL, &cfg, &out, "disk must not be NULL");
    ALL4F(&bh, &dk, &cfg, 0, &out, NULL, &eo, "params must not be NULL");
    {
        const int ks[] = {0, -1, BHRT_EMIT_MAX_CROSSINGS + 1, INT_MAX};
        for (int i = 0; i < 4; i++) {
            const bhrt_kerr_emit_params p = {ks[i], 3.0, 1.0};
            ALL4F(&bh, &dk, &cfg, 0, &out, &p, &eo, "max_crossings");
        }
        const double bad[] = {-1e-300, -1.0, NAN, INFINITY, -INFINITY};
        for (int i = 0; i < 5; i++) {
            const bhrt_kerr_emit_params pq = {K, bad[i], 1.0}, pg = {K, 3.0, bad[i]};
            ALL4F(&bh, &dk, &cfg, 0, &out, &pq, &eo, "emissivity_index");
            ALL4F(&bh, &dk, &cfg, 0, &out, &pg, &eo, "gain");
        }
        ALL4F(&bh, &dk, &cfg, BHRT_FLAG_DOPPLER, &out, &ep, &eo, "BHRT_FLAG_DOPPLER");
        bhrt_frame_soa none;
        memset(&none, 0, sizeof none);
        const bhrt_kerr_emit_out nothing = {NULL, NULL, NULL, NULL};
        ALL4F(&bh, &dk, &cfg, 0, &none, &ep, &nothing, "no output");
        ALL4F(&bh, &dk, &cfg, 0, &none, &ep, NULL, "no output");
    }
    /* (long)K * n > INT_MAX: K = 4 planes of a 32768 x 16385 frame, and of as many rays */
    {
        const bhrt_kerr_emit_params p4 = {4, 3.0, 1.0};
        REFUSED(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &cam, 32768, 16385, NULL, 0, &out, NULL,
                                            &p4, &eo, NULL), "INT_MAX");
        REFUSED(bhrt_kerr_emit_rays_device(rays, 32768 * 16385, &bh, &dk, &cfg, 0, &out, NULL, &p4,
                                           &eo, NULL), "INT_MAX");
    }
    /* an origin without a static observer: inside the horizon, inside the ergosphere */
    {
        const Vector3D bad[] = {{0.5, 0.0, 0.0}, {1.9, 0.0, 0.0}, {NAN, 0.0, 0.0}};
        for (int i = 0; i < 3; i++) {
            bhrt_camera c = cam;
            c.position = bad[i];
            REFUSED(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &c, W, H, NULL, 0, &out, NULL, &ep,
                                                &eo, NULL), "no static observer");
            REFUSED(bhrt_kerr_emit_frame(&bh, &dk, &cfg, &c, W, H, 0, &out, NULL, &ep, &eo),
                    "no static observer");
            const Vector3D keep = rays[N - 1].origin;
            rays[N - 1].origin = bad[i];
            REFUSED(bhrt_kerr_emit_rays(rays, N, &bh, &dk, &cfg, 0, &out, NULL, &ep, &eo),
                    "of ray 1322");
            rays[N - 1].origin = keep;
        }
    }
    REFUSED(bhrt_kerr_emit_frame(&bh, &dk, &cfg, NULL, W, H, 0, &out, NULL, &ep, &eo), "camera");
    REFUSED(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &cam, 0, H, NULL, 0, &out, NULL, &ep, &eo,
                                        NULL), "invalid size");
    {
        const bhrt_rows badrows = {0, 0, 3};
        REFUSED(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &cam, W, H, &badrows, 0, &out, NULL,
                                            &ep, &eo, NULL), "row sharding");
    }
    REFUSED(bhrt_kerr_emit_rays_device(rays, 0, &bh, &dk, &cfg, 0, &out, NULL, &ep, &eo, NULL),
            "n = 0");
    REFUSED(bhrt_kerr_emit_rays(NULL, N, &bh, &dk, &cfg, 0, &out, NULL, &ep, &eo),
            "rays must not be NULL");
    {
        double g = -7.0;
        BlackHoleParams b = bh;
        b.spin = 1.0;
        REFUSED(bhrt_kerr_disk_redshift(NULL, 6.0, 1.0, 0.0, &g), "NULL");
        REFUSED(bhrt_kerr_disk_redshift(&bh, 6.0, 1.0, 0.0, NULL), "NULL");
        REFUSED(bhrt_kerr_disk_redshift(&b, 6.0, 1.0, 0.0, &g), "spin");
        CHECK(g == -7.0, "a refused redshift call wrote %g", g);
    }
    CHECK(g_hip == 0 && g_query == 0, "refusals made %ld HIP calls, %ld queries", g_hip, g_query);
    /* the sky flag without a bound map: the current device's query and nothing else */
    g_hip = g_query = 0;
    REFUSED(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &cam, W, H, NULL, BHRT_FLAG_SKY, &out, NULL,
                                        &ep, &eo, NULL), "no sky map is bound");
    CHECK(g_hip == 0, "the sky refusal made %ld HIP calls", g_hip);
    for (int i = 0; i < N; i++)
        if (res[i] != -7 || hx[i] != -7.0 || sx[i] != -7.0 || col[i] != -7.0 || dg[i] != -7.0 ||
            rj[i] != -7 || cnt[i] != -7 || inten[i] != -7.0 || rad[i] != -7.0 ||
            rad[(K - 1) * N + i] != -7.0 || red[i] != -7.0 || red[(K - 1) * N + i] != -7.0) {
            CHECK(0, "a refusal wrote element %d", i);
            break;
        }
    CHECK(g_launches == 0, "a refusal launched");

    /* ---- 2. the redshift on the host: no HIP call ---- */
    {
        g_hip = g_query = 0;
        BlackHoleParams s0;
        initialize_black_hole_params(&s0, 1.0, 0.0, 0.0);
        double g = -1.0;
        /* spin 0, L_z = 0: sqrt(1 - 3 M / r) / E, all exactly rounded operations */
        CHECK(bhrt_kerr_disk_redshift(&s0, 4.0, 0.5, 0.0, &g) == 0 && g == sqrt(0.25) / 0.5,
              "g = %.17g", g);
        CHECK(bhrt_kerr_disk_redshift(&s0, 2.5, 1.0, 0.0, &g) == 0 && g == 0.0,
              "inside the photon orbit g = %g", g);
        CHECK(bhrt_kerr_disk_redshift(&s0, 6.0, 1.0, -1e9, &g) == 0 && g == 0.0,
              "E + Omega L_z <= 0: g = %g", g);
        CHECK(bhrt_kerr_disk_redshift(&bh, NAN, 1.0, 0.0, &g) == 0 && g == 0.0, "NaN radius: %g", g);
        CHECK(g_hip == 0 && g_query == 0, "the redshift made %ld HIP calls", g_hip + g_query);
    }

    /* ---- 3. a whole frame on the device: what the launch carries ---- */
    void *d_res = NULL, *d_cnt = NULL, *d_rad = NULL, *d_red = NULL, *d_int = NULL, *d_rays = NULL,
         *d_rj = NULL;
    if (__real_hipMalloc(&d_res, 4 * N) || __real_hipMalloc(&d_cnt, 4 * N) ||
        __real_hipMalloc(&d_rad, 8 * K * N) || __real_hipMalloc(&d_red, 8 * K * N) ||
        __real_hipMalloc(&d_int, 8 * N) || __real_hipMalloc(&d_rays, sizeof(Ray) * N) ||
        __real_hipMalloc(&d_rj, 4 * N))
        abort();
    memcpy(d_rays, rays, sizeof(Ray) * N);
    bhrt_frame_soa dout;
    memset(&dout, 0, sizeof dout);
    dout.result = (int32_t*)d_res;
    const bhrt_kerr_rk45_diag ddiag = {NULL, NULL, (int*)d_rj};
    const bhrt_kerr_emit_out deo = {(int*)d_cnt, (double*)d_rad, (double*)d_red, (double*)d_int};
    CHECK(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &cam, W, H, NULL, 0, &dout, &ddiag, &ep, &deo,
                                      NULL) == 0 && g_launches == 1, "frame: %s", bhrt_last_error());
    CHECK(g_kp.src == BHRT_SRC_CAMERA && g_kp.n == N && g_ek.rk.k.nrows == H &&
          g_ek.rk.k.tiles_x == 7 && g_ek.rk.k.ntiles == 7 * 4, "frame geometry");
    CHECK(g_ek.max_crossings == K && g_ek.q == 3.0 && g_ek.gain == 1.5 && g_ek.spin_a == 0.9 &&
          g_ek.rk.k.a == -0.9 && g_ek.rk.tol == 1e-8 && g_ek.rk.k.dt == 0.25, "emission constants");
    CHECK(g_ek.rk.k.has_disk == 1 && g_kp.sc.has_disk == 1 && g_kp.sc.disk_in == 2.4 &&
          g_kp.sc.flags == 0, "disk constants");
    CHECK(g_ek.out.count == (int*)d_cnt && g_ek.out.radius == (double*)d_rad &&
          g_ek.out.redshift == (double*)d_red && g_ek.out.intensity == (double*)d_int &&
          g_ek.rk.rejected == (int*)d_rj && g_ek.rk.k.h_residual == NULL, "output pointers");
    CHECK(((int*)d_cnt)[7] == 3 && ((double*)d_rad)[2 * N + 7] == 7.25, "the launch's outputs");
    /* a row shard, emission outputs alone (no frame field, a NULL diag) */
    {
        bhrt_frame_soa none;
        memset(&none, 0, sizeof none);
        const bhrt_rows rows = {8, 1, 3};
        const bhrt_kerr_emit_out only = {NULL, NULL, NULL, (double*)d_int};
        const bhrt_kerr_emit_params p1 = {1, 0.0, 0.0};
        CHECK(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &cam, W, H, &rows, 0, &none,
                                          NULL, &p1, &only, NULL) == 0 && g_launches == 2,
              "shard: %s", bhrt_last_error());
        CHECK(g_kp.n == 8 * W && g_ek.rk.k.nrows == 8 && g_ek.rk.k.ntiles == 7 &&
              g_kp.cam.rows.shard == 1 && g_ek.max_crossings == 1 && g_ek.q == 0.0 &&
              g_ek.gain == 0.0 && g_ek.out.count == NULL && g_ek.out.radius == NULL,
              "shard launch");
        /* a frame field alone, a NULL emit struct */
        CHECK(bhrt_kerr_emit_frame_device(&bh, &dk, &cfg, &cam, W, H, NULL, 0, &dout, NULL, &ep, NULL,
                                          NULL) == 0 && g_ek.out.intensity == NULL &&
              g_ek.out.count == NULL, "no emit struct: %s", bhrt_last_error());
    }
    /* a ray array */
    CHECK(bhrt_kerr_emit_rays_device((const Ray*)d_rays, N - 3, &bh, &dk, &cfg, 0, &dout, &ddiag, &ep,
                                     &deo, NULL) == 0 && g_kp.src == BHRT_SRC_RAYS &&
          g_kp.rays == (const Ray*)d_rays && g_kp.n == N - 3, "rays: %s", bhrt_last_error());
    /* the largest K, and the bounds of q and gain are taken */
    {
        const bhrt_kerr_emit_params p4 = {BHRT_EMIT_MAX_CROSSINGS, 0.0, 0.0};
        const bhrt_kerr_emit_out only = {(int*)d_cnt, NULL, NULL, NULL};
        CHECK(bhrt_kerr_emit_rays_device((const Ray*)d_rays, 5, &bh, &dk, &cfg, 0, &dout, NULL, &p4,
                                         &only, NULL) == 0 && g_ek.max_crossings == 4,
              "K = 4: %s", bhrt_last_error());
    }

    /* ---- 4. the host forms: round trips; unwritten elements keep what they held ---- */
    long l0 = g_launches;
    CHECK(bhrt_kerr_emit_frame(&bh, &dk, &cfg, &cam, W, H, 0, &out, &diag, &ep, &eo) == 0 &&
          g_launches == l0 + 1 && g_kp.n == N && g_kp.src == BHRT_SRC_CAMERA, "host frame: %s",
          bhrt_last_error());
    for (int i = 0; i < N; i++) {
        int ok = res[i] == i % 5 && hx[i] == i + 0.25 && sx[i] == (i % 2 ? -7.0 : -(double)i) &&
                 col[i] == 0.125 && dg[i] == 1e-6 * i && rj[i] == i % 3 && cnt[i] == i % (K + 1) &&
                 inten[i] == 0.5 * i;
        for (int k = 0; k < K; k++) {
            const double want = k < i % (K + 1) ? i + k / 8.0 : -7.0;
            ok = ok && rad[k * N + i] == want && red[k * N + i] == (want == -7.0 ? -7.0 : -want);
        }
        if (!ok) {
            CHECK(0, "host frame element %d: %d %g %d %g %g", i, res[i], hx[i], cnt[i], rad[i],
                  red[i]);
            break;
        }
    }
    for (int i = 0; i < N; i++) {
        res[i] = cnt[i] = -7;
        inten[i] = -7.0;
        for (int k = 0; k < K; k++) rad[k * N + i] = red[k * N + i] = -7.0;
    }
    {
        bhrt_frame_soa o;
        memset(&o, 0, sizeof o);
        o.result = res;
        const bhrt_kerr_emit_out some = {cnt, NULL, red, NULL};
        CHECK(bhrt_kerr_emit_rays(rays, N - 1, &bh, &dk, &cfg, 0, &o, NULL, &ep, &some) == 0 &&
              g_kp.n == N - 1 && g_kp.src == BHRT_SRC_RAYS && g_ek.out.radius == NULL &&
              g_ek.out.intensity == NULL && g_ek.rk.rejected == NULL, "host rays: %s",
              bhrt_last_error());
        CHECK(memcmp(g_kp.rays, rays, sizeof(Ray) * (N - 1)) == 0, "the uploaded rays");
        /* planes are [K][n] with n = N - 1 here */
        const int n1 = N - 1, i = N - 2;
        CHECK(res[i] == i % 5 && cnt[i] == i % (K + 1) && res[N - 1] == -7 && cnt[N - 1] == -7 &&
              rad[i] == -7.0 && inten[i] == -7.0, "host rays' elements");
        CHECK(red[0 * n1 + 5] == -5.0 && red[1 * n1 + 5] == -7.0 && red[1 * n1 + 6] == -6.125 &&
              red[2 * n1 + 7] == -7.25, "host rays' redshift planes");
        CHECK(bhrt_kerr_emit_rays(rays, 1, &bh, &dk, &cfg, 0, &o, NULL, &ep, NULL) == 0 &&
              g_kp.n == 1, "one ray");
    }
    /* the statistics count emission launches as trace launches */
    {
        bhrt_stats st;
        CHECK(bhrt_get_stats(&st, 1) == 0 && st.launches == (uint64_t)g_launches && st.rays > 0 &&
              st.iterations == 3 * st.rays, "stats: %llu launches, %llu rays, %llu iterations",
              (unsigned long long)st.launches, (unsigned long long)st.rays,
              (unsigned long long)st.iterations);
    }
    __real_hipFree(d_res);
    __real_hipFree(d_cnt);
    __real_hipFree(d_rad);
    __real_hipFree(d_red);
    __real_hipFree(d_int);
    __real_hipFree(d_rays);
    __real_hipFree(d_rj);
    free(res);
    free(hx);
    free(sx);
    free(col);
    free(dg);
    free(rj);
    free(cnt);
    free(rad);
    free(red);
    free(inten);
    free(rays);
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld refusals, %ld emission launches)\n", g_refusals, g_launches);
    return 0;
}
