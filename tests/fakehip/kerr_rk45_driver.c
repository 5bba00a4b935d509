/* kerr_rk45_driver.c -- adaptive physical geodesics (kerr_rk45.c and kerr.c, whose checks it
 * shares, over the HOST_CORE files) on SIMULATED devices (fake_hip.c), built by
 * tests/test_kerr_rk45_cpu.py under ASan+UBSan as a stand-alone program.
 *
 * The adaptive launcher is a stub: it checks that every buffer of the launch lies on the simulated
 * device, records the launch's parameters and fills the outputs with an encoding of the ray id;
 * the fixed-step launcher aborts, for no adaptive call may reach it. The HIP entry points the
 * host code can reach are counted through the linker's --wrap, so "no HIP call" is checked, not
 * assumed.
 *
 * Checked: every refusal of include/bhrt_api.h "Physical geodesics, adaptive steps" -- those of
 * the fixed-step calls and the tolerance's -- with zero HIP calls (the current device's query
 * aside, for the one refusal that needs it) and nothing written, counted and printed; the
 * constants a launch carries (the tolerance, the first trial step, the tile counts of whole
 * frames and shards); ray arrays; the host forms' round trips with the rejected plane, sky_*
 * elements kept where the kernel does not write them; the statistics. Test infrastructure only. */
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
static bhrt_kerr_k g_kk;
static bhrt_kerr_rk45_k g_rk;

int bhrt_launch_kerr(const bhrt_kparams* kp, const bhrt_kerr_k* kk, void* stream, void* ev0,
                     void* ev1) {
    (void)kp; (void)kk; (void)stream; (void)ev0; (void)ev1;
    fprintf(stderr, "an adaptive call reached the fixed-step launcher\n");
    abort();
}

int bhrt_launch_kerr_rk45(const bhrt_kparams* kp, const bhrt_kerr_rk45_k* rk, void* stream,
                          void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    const bhrt_kerr_k* kk = &rk->k;
    const size_t n = (size_t)kp->n;
    on_device(kp->ctl, 8 * 16, "control block");
    if (kp->src == BHRT_SRC_RAYS) on_device(kp->rays, sizeof(Ray) * n, "rays");
    static const size_t fsize[15] = {4, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 16, 4};
    void* const* f = (void* const*)&kp->out;
    for (int i = 0; i < 15; i++)
        if (f[i]) on_device(f[i], fsize[i] * n, "an output field");
    if (kk->h_residual) on_device(kk->h_residual, 8 * n, "h_residual");
    if (kk->lz_drift) on_device(kk->lz_drift, 8 * n, "lz_drift");
    if (rk->rejected) on_device(rk->rejected, 4 * n, "rejected");
    g_kp = *kp;
    g_kk = *kk;
    g_rk = *rk;
    for (size_t i = 0; i < n; i++) {
        if (kp->out.result) kp->out.result[i] = (int32_t)(i % 5);
        if (kp->out.steps) kp->out.steps[i] = (int32_t)i;
        if (kp->out.hit_x) kp->out.hit_x[i] = (double)i + 0.25;
        if (kp->out.distance) kp->out.distance[i] = (double)i + 0.5;
        if (kp->out.sky_x && i % 2 == 0) kp->out.sky_x[i] = -(double)i; /* (odd ones not written) */
        if (kp->out.rgb_r) kp->out.rgb_r[i] = kp->out.rgb_g[i] = kp->out.rgb_b[i] = 0.125;
        if (kp->out.rgba8) memset(kp->out.rgba8 + 4 * i, 0x11, 4);
        if (kk->h_residual) kk->h_residual[i] = 1e-6 * (double)i;
        if (kk->lz_drift) kk->lz_drift[i] = 2e-6 * (double)i;
        if (rk->rejected) rk->rejected[i] = (int)(i % 3);
    }
    kp->ctl[1] += n;
    kp->ctl[2] += 3 * n;
    g_launches++;
    return 0;
}

int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)kp; (void)stream; (void)ev0; (void)ev1;
    fprintf(stderr, "an adaptive Kerr call reached the parity trace launcher\n");
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
    cfg.tolerance = 1e-6;
    enum { W = 49, H = 27, N = W * H };

    /* poisoned host outputs: a refusal writes nothing */
    int32_t* res = (int32_t*)malloc(4 * N);
    double* hx = (double*)malloc(8 * N);
    double* sx = (double*)malloc(8 * N);
    double* col = (double*)malloc(3 * 8 * N);
    double* dg = (double*)malloc(2 * 8 * N);
    int* rj = (int*)malloc(4 * N);
    Ray* rays = (Ray*)malloc(sizeof(Ray) * N);
    for (int i = 0; i < N; i++) {
        res[i] = -7;
        hx[i] = sx[i] = -7.0;
        col[i] = col[N + i] = col[2 * N + i] = -7.0;
        dg[i] = dg[N + i] = -7.0;
        rj[i] = -7;
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
    const bhrt_kerr_rk45_diag diag = {dg, dg + N, rj};

    /* ---- 1. refusals: zero HIP calls, not even the query; nothing written ---- */
    g_hip = g_query = 0;
#define REFUSED(call, needle)                                                          \
    do {                                                                               \
        g_refusals++;                                                                  \
        CHECK((call) == -1 && has(needle), "%s: rc or message: %s", #call, bhrt_last_error()); \
    } while (0)
#define ALL4(BH, DK, CFG, OUT, needle)                                                 \
    do {                                                                               \
        REFUSED(bhrt_kerr_rk45_frame_device(BH, DK, CFG, &cam, W, H, NULL, 0, OUT, &diag, NULL), needle); \
        REFUSED(bhrt_kerr_rk45_frame(BH, DK, CFG, &cam, W, H, 0, OUT, &diag), needle);       \
        REFUSED(bhrt_kerr_rk45_rays_device(rays, N, BH, DK, CFG, 0, OUT, &diag, NULL), needle); \
        REFUSED(bhrt_kerr_rk45_rays(rays, N, BH, DK, CFG, 0, OUT, &diag), needle);           \
    } while (0)
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
        /* the tolerance: finite and within [1e-12, 1e-2]; both bounds are taken (section 2) */
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
        o = out;
        o.rgb_r = o.rgb_g = NULL;
        ALL4(&bh, &dk, &cfg, &o, "rgb_r/g/b");
    }
    /* an origin without a static observer: inside the horizon, inside the ergosphere */
    {
        const Vector3D bad[] = {{0.5, 0.0, 0.0}, {1.0, 1.0, 0.0}, {1.9, 0.0, 0.0}, {NAN, 0.0, 0.0}};
        for (int i = 0; i < 4; i++) {
            bhrt_camera c = cam;
            c.position = bad[i];
            REFUSED(bhrt_kerr_rk45_frame_device(&bh, &dk, &cfg, &c, W, H, NULL, 0, &out, NULL, NULL),
                    "no static observer");
            REFUSED(bhrt_kerr_rk45_frame(&bh, &dk, &cfg, &c, W, H, 0, &out, NULL), "no static observer");
            const Vector3D keep = rays[N - 1].origin;
            rays[N - 1].origin = bad[i];
            REFUSED(bhrt_kerr_rk45_rays(rays, N, &bh, &dk, &cfg, 0, &out, NULL), "of ray 1322");
            rays[N - 1].origin = keep;
        }
    }
    REFUSED(bhrt_kerr_rk45_frame_device(&bh, &dk, &cfg, NULL, W, H, NULL, 0, &out, NULL, NULL), "camera");
    REFUSED(bhrt_kerr_rk45_frame(&bh, &dk, &cfg, NULL, W, H, 0, &out, NULL), "camera");
    REFUSED(bhrt_kerr_rk45_frame_device(&bh, &dk, &cfg, &cam, 0, H, NULL, 0, &out, NULL, NULL), "invalid size");
    REFUSED(bhrt_kerr_rk45_frame(&bh, &dk, &cfg, &cam, W, -1, 0, &out, NULL), "invalid size");
    {
        const bhrt_rows badrows = {0, 0, 3}, badshard = {8, 3, 3};
        REFUSED(bhrt_kerr_rk45_frame_device(&bh, &dk, &cfg, &cam, W, H, &badrows, 0, &out, NULL, NULL), "row sharding");
        REFUSED(bhrt_kerr_rk45_frame_device(&bh, &dk, &cfg, &cam, W, H, &badshard, 0, &out, NULL, NULL), "row sharding");
    }
    REFUSED(bhrt_kerr_rk45_rays_device(rays, 0, &bh, &dk, &cfg, 0, &out, NULL, NULL), "n = 0");
    REFUSED(bhrt_kerr_rk45_rays(rays, -5, &bh, &dk, &cfg, 0, &out, NULL), "n = -5");
    REFUSED(bhrt_kerr_rk45_rays_device(NULL, N, &bh, &dk, &cfg, 0, &out, NULL, NULL), "rays must not be NULL");
    REFUSED(bhrt_kerr_rk45_rays(NULL, N, &bh, &dk, &cfg, 0, &out, NULL), "rays must not be NULL");
    CHECK(g_hip == 0 && g_query == 0, "refusals made %ld HIP calls, %ld queries", g_hip, g_query);
    /* the sky flag without a bound map: the current device's query and nothing else */
    g_hip = g_query = 0;
    REFUSED(bhrt_kerr_rk45_frame_device(&bh, &dk, &cfg, &cam, W, H, NULL, BHRT_FLAG_SKY, &out, NULL, NULL),
            "no sky map is bound");
    REFUSED(bhrt_kerr_rk45_rays(rays, N, &bh, &dk, &cfg, BHRT_FLAG_SKY, &out, NULL), "no sky map is bound");
    CHECK(g_hip == 0, "the sky refusal made %ld HIP calls", g_hip);
    for (int i = 0; i < N; i++)
        if (res[i] != -7 || hx[i] != -7.0 || sx[i] != -7.0 || col[i] != -7.0 || dg[i] != -7.0 ||
            dg[N + i] != -7.0 || rj[i] != -7) {
            CHECK(0, "a refusal wrote element %d", i);
            break;
        }
    CHECK(g_launches == 0, "a refusal launched");
    /* ---- 2. a whole frame on the device: the constants and the tiles of the launch ---- */
    void *d_res = NULL, *d_hx = NULL, *d_sx = NULL, *d_h = NULL, *d_rays = NULL, *d_rj = NULL;
    if (__real_hipMalloc(&d_res, 4 * N) || __real_hipMalloc(&d_hx, 8 * N) ||
        __real_hipMalloc(&d_sx, 8 * N) || __real_hipMalloc(&d_h, 8 * N) ||
        __real_hipMalloc(&d_rays, sizeof(Ray) * N) || __real_hipMalloc(&d_rj, 4 * N))
        abort();
    memcpy(d_rays, rays, sizeof(Ray) * N);
    bhrt_frame_soa dout;
    memset(&dout, 0, sizeof dout);
    dout.result = (int32_t*)d_res;
    dout.hit_x = (double*)d_hx;
    dout.sky_x = (double*)d_sx;
    const bhrt_kerr_rk45_diag ddiag = {(double*)d_h, NULL, (int*)d_rj};
    CHECK(bhrt_kerr_rk45_frame_device(&bh, &dk, &cfg, &cam, W, H, NULL, BHRT_FLAG_DOPPLER, &dout, &ddiag,
                                 NULL) == 0 && g_launches == 1, "frame: %s", bhrt_last_error());
    CHECK(g_kp.src == BHRT_SRC_CAMERA && g_kp.n == N && g_kk.nrows == H && g_kk.tiles_x == 7 &&
          g_kk.ntiles == 7 * 4, "frame geometry n %d rows %d tiles %d x of %d", g_kp.n, g_kk.nrows,
          g_kk.tiles_x, g_kk.ntiles);
    CHECK(g_kk.a == -0.9 && g_kk.a2 == 0.9 * 0.9 && g_kk.M == 1.0 && g_kk.two_m == 2.0 &&
          g_kk.eight_m == 8.0 && g_kk.r_plus == 1.0 + sqrt(1.0 - 0.9 * 0.9), "spin constants");
    CHECK(g_kk.dt == 0.25 && g_kk.max_dist == 60.0 && g_kk.max_steps == 2000 && g_kk.has_disk == 1 &&
          g_kk.disk_lo == 2.4 * 2.4 + 0.9 * 0.9 && g_kk.disk_hi == 12.0 * 12.0 + 0.9 * 0.9,
          "scene constants");
    CHECK(g_kp.sc.flags == BHRT_FLAG_DOPPLER && g_kp.sc.disk_in == 2.4 && g_kp.sc.disk_out == 12.0 &&
          g_kp.sc.rs == bh.schwarzschild_radius && g_kp.sc.has_disk == 1, "colour constants");
    CHECK(g_kp.cam.pos[1] == -18.0 && g_kp.cam.pos[2] == 4.0 && g_kp.cam.off_x == 0.5 &&
          g_kp.cam.off_y == 0.5 && g_kp.cam.width == W && g_kp.cam.height == H &&
          g_kp.cam.rows.num_shards == 1, "camera block");
    CHECK(g_kk.h_residual == (double*)d_h && g_kk.lz_drift == NULL && g_rk.rejected == (int*)d_rj,
          "diag pointers");
    CHECK(g_rk.tol == 1e-6 && ((int*)d_rj)[7] == 1, "the tolerance and the rejected plane");
    CHECK(((int32_t*)d_res)[7] == 2 && ((double*)d_hx)[7] == 7.25, "the launch's outputs");
    /* the sub-pixel offset and a row shard: 27 rows in blocks of 8, shard 1 of 3 has rows 8..15 */
    {
        bhrt_camera c = cam;
        c.use_offset = 1;
        c.offset_x = 0.25;
        c.offset_y = 0.75;
        const bhrt_rows rows = {8, 1, 3};
        CHECK(bhrt_kerr_rk45_frame_device(&bh, NULL, &cfg, &c, W, H, &rows, 0, &dout, NULL, NULL) == 0 &&
              g_launches == 2, "shard: %s", bhrt_last_error());
        CHECK(g_kp.n == 8 * W && g_kk.nrows == 8 && g_kk.ntiles == 7 && g_kp.cam.rows.shard == 1 &&
              g_kp.cam.rows.num_shards == 3 && g_kp.cam.rows.row_block == 8 && g_kp.cam.off_x == 0.25 &&
              g_kp.cam.off_y == 0.75 && g_kk.has_disk == 0 && g_kp.sc.has_disk == 0, "shard launch");
        const bhrt_rows last = {8, 0, 3}; /* rows 0..7 and 24..26: 11 rows, two rows of tiles */
        CHECK(bhrt_kerr_rk45_frame_device(&bh, NULL, &cfg, &c, W, H, &last, 0, &dout, NULL, NULL) == 0 &&
              g_kk.nrows == 11 && g_kk.ntiles == 14 && g_kp.n == 11 * W, "ragged shard");
    }
    /* a ray array */
    CHECK(bhrt_kerr_rk45_rays_device((const Ray*)d_rays, N - 3, &bh, &dk, &cfg, 0, &dout, &ddiag, NULL) == 0 &&
          g_kp.src == BHRT_SRC_RAYS && g_kp.rays == (const Ray*)d_rays && g_kp.n == N - 3,
          "rays: %s", bhrt_last_error());
    CHECK(((int32_t*)d_res)[N - 1] == (N - 1) % 5, "element beyond n written");
    {
        SimulationConfig c = cfg; /* zero steps and an infinite distance are scenes, not refusals */
        c.max_integration_steps = 0;
        c.max_ray_distance = INFINITY;
        CHECK(bhrt_kerr_rk45_rays_device((const Ray*)d_rays, 5, &bh, NULL, &c, 0, &dout, NULL, NULL) == 0 &&
              g_kk.max_steps == 0 && isinf(g_kk.max_dist), "steps 0: %s", bhrt_last_error());
    }

    /* the tolerance's bounds are taken, and time_step travels as the first trial step */
    {
        const double ok[] = {1e-12, 1e-2}; /* the bounds themselves are scenes */
        for (int i = 0; i < 2; i++) {
            SimulationConfig c = cfg;
            c.tolerance = ok[i];
            c.time_step = 3.0; /* the first trial step, as given */
            const long before = g_launches;
            CHECK(bhrt_kerr_rk45_frame_device(&bh, &dk, &c, &cam, W, H, NULL, 0, &dout, NULL, NULL) == 0 &&
                  g_launches == before + 1 && g_rk.tol == ok[i] && g_kk.dt == 3.0 &&
                  g_rk.rejected == NULL && g_kk.h_residual == NULL, "tolerance bound %g: %s", ok[i],
                  bhrt_last_error());
        }
    }

    /* ---- 3. the host forms: round trips; sky_* keeps what the kernel does not write ---- */
    long l0 = g_launches;
    CHECK(bhrt_kerr_rk45_frame(&bh, &dk, &cfg, &cam, W, H, 0, &out, &diag) == 0 && g_launches == l0 + 1 &&
          g_kp.n == N && g_kp.src == BHRT_SRC_CAMERA, "host frame: %s", bhrt_last_error());
    for (int i = 0; i < N; i++)
        if (res[i] != i % 5 || hx[i] != i + 0.25 || sx[i] != (i % 2 ? -7.0 : -(double)i) ||
            col[i] != 0.125 || col[2 * N + i] != 0.125 || dg[i] != 1e-6 * i || dg[N + i] != 2e-6 * i ||
            rj[i] != i % 3) {
            CHECK(0, "host frame element %d: %d %g %g %g %g", i, res[i], hx[i], sx[i], col[i], dg[i]);
            break;
        }
    for (int i = 0; i < N; i++) res[i] = -7, hx[i] = -7.0, dg[i] = -7.0, rj[i] = -7;
    {
        bhrt_frame_soa o;
        memset(&o, 0, sizeof o);
        o.result = res;
        o.hit_x = hx;
        const bhrt_kerr_rk45_diag only_h = {dg, NULL, NULL};
        CHECK(bhrt_kerr_rk45_rays(rays, N - 1, &bh, NULL, &cfg, 0, &o, &only_h) == 0 && g_kp.n == N - 1 &&
              g_kp.src == BHRT_SRC_RAYS && g_kk.lz_drift == NULL, "host rays: %s", bhrt_last_error());
        CHECK(memcmp(g_kp.rays, rays, sizeof(Ray) * (N - 1)) == 0, "the uploaded rays");
        CHECK(res[N - 2] == (N - 2) % 5 && hx[N - 2] == N - 2 + 0.25 && dg[N - 2] == 1e-6 * (N - 2) &&
              res[N - 1] == -7 && hx[N - 1] == -7.0 && dg[N - 1] == -7.0 && rj[0] == -7 &&
              g_rk.rejected == NULL, "host rays' elements");
        const bhrt_kerr_rk45_diag only_r = {NULL, NULL, rj};
        CHECK(bhrt_kerr_rk45_rays(rays, N - 1, &bh, NULL, &cfg, 0, &o, &only_r) == 0 &&
              g_kk.h_residual == NULL && rj[N - 2] == (N - 2) % 3 && rj[N - 1] == -7,
              "rejected alone: %s", bhrt_last_error());
        CHECK(bhrt_kerr_rk45_rays(rays, 1, &bh, NULL, &cfg, 0, &o, NULL) == 0 && g_kp.n == 1, "one ray");
    }
    /* the statistics count Kerr launches as trace launches */
    {
        bhrt_stats st;
        CHECK(bhrt_get_stats(&st, 1) == 0 && st.launches == (uint64_t)g_launches && st.rays > 0 &&
              st.iterations == 3 * st.rays, "stats: %llu launches, %llu rays, %llu iterations",
              (unsigned long long)st.launches, (unsigned long long)st.rays,
              (unsigned long long)st.iterations);
    }
    __real_hipFree(d_res);
    __real_hipFree(d_hx);
    __real_hipFree(d_sx);
    __real_hipFree(d_h);
    __real_hipFree(d_rays);
    __real_hipFree(d_rj);
    free(res);
    free(hx);
    free(sx);
    free(col);
    free(dg);
    free(rj);
    free(rays);
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld refusals, %ld adaptive launches)\n", g_refusals, g_launches);
    return 0;
}
