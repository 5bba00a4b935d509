/* paths_driver.c -- the host form of batched photon paths (paths.c bhrt_trace_paths, over
 * the HOST_CORE files) on a SIMULATED device (fake_hip.c), built by tests/test_paths_cpu.py under
 * ASan+UBSan as a stand-alone program.
 *
 * The path launcher is a stub that checks every launch buffer against the simulated device and
 * fills the device arrays from host code: ray i (its id rides in origin.x, so the upload is
 * checked too) stores want_count(i) points whose coordinates encode (i, j, c); the trace
 * launcher, which libbhrt queues behind it for the hit records, an encoding of i in every hit
 * field. The program runs batches of 1 and 5 rays with ragged counts through each
 * readback form (one rectangle, the staged rectangle, one copy per ray) and checks every stored
 * point, every count and hit, and that every host element beyond count[i] keeps its sentinel.
 * Test infrastructure only. */
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

static void on_device(const void* p, size_t n, const char* what) {
    if (!p) return;
    const int k = fakehip_kind_of(p, n);
    if (k != fakehip_current_device()) {
        fprintf(stderr, "launch buffer %s (%zu B) is memory kind %d, launching on device %d\n",
                what, n, k, fakehip_current_device());
        abort();
    }
}

static int g_full;     /* every ray stores max_positions points */
static long g_launches;
static int want_count(int i, int P) { return g_full ? P : 1 + (i * 3 + 2) % P; }
static double enc(int i, int j, int c) { return i * 1000.0 + j * 4.0 + c + 0.5; }
static double enc_hit(int f, int i) { return i * 16.0 + f + 0.25; }

int bhrt_launch_paths(const bhrt_kparams* kp, const bhrt_paths_k* pk, void* stream, void* ev0,
                      void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    const size_t n = (size_t)kp->n, P = (size_t)pk->max_positions;
    on_device(kp->rays, sizeof(Ray) * n, "rays");
    on_device(kp->ctl, 8 * 8, "control block");
    on_device(pk->out.xyz, sizeof(Vector3D) * n * P, "xyz");
    on_device(pk->out.xyz32, 12 * n * P, "xyz32");
    on_device(pk->out.count, 4 * n, "count");
    void* const* out = (void* const*)&kp->out;
    for (int f = 0; f < 15; f++)
        if (out[f]) {
            fprintf(stderr, "path launch with a hit field (the hits are the trace launch's)\n");
            abort();
        }
    if (kp->ctl[0] != 0) {
        fprintf(stderr, "claim counter not zero at launch\n");
        abort();
    }
    for (size_t i = 0; i < n; i++) {
        if (kp->rays[i].origin.x != (double)i) {
            fprintf(stderr, "ray %zu was not uploaded\n", i);
            abort();
        }
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
    }
    kp->ctl[0] = (n + 63) / 64 * 64; /* (the kernel's claims) */
    kp->ctl[1] += n;                 /* rays */
    g_launches++;
    return 0;
}

/* the trace launch behind a path launch whose caller asked for the hits: an encoding of the
 * ray in every hit field */
static long g_traces;
int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    const size_t n = (size_t)kp->n;
    static const size_t fsize[10] = {4, 4, 8, 8, 8, 8, 8, 8, 8, 8};
    void* const* out = (void* const*)&kp->out;
    for (int f = 0; f < 10; f++) on_device(out[f], fsize[f] * n, "hit field");
    for (int f = 10; f < 15; f++)
        if (out[f]) {
            fprintf(stderr, "hits launch with a colour field\n");
            abort();
        }
    on_device(kp->rays, sizeof(Ray) * n, "rays");
    on_device(kp->init, (size_t)(BHRT_INIT_FIELDS + 1) * 8 * n, "init table");
    on_device(kp->ctl, 8 * 8, "control block");
    if (kp->sc.flags != 0 || kp->src != BHRT_SRC_RAYS) {
        fprintf(stderr, "hits launch is not a plain ray-array trace\n");
        abort();
    }
    for (size_t i = 0; i < n; i++) {
        if (kp->out.result) kp->out.result[i] = (int)(i % 5);
        if (kp->out.steps) kp->out.steps[i] = (int)i + 3;
        double* d[8] = {kp->out.hit_x, kp->out.hit_y, kp->out.hit_z, kp->out.distance,
                        kp->out.time_dilation, kp->out.sky_x, kp->out.sky_y, kp->out.sky_z};
        for (int f = 0; f < 8; f++)
            if (d[f]) d[f][i] = enc_hit(f, (int)i);
    }
    kp->ctl[1] += n;
    g_traces++;
    return 0;
}
/* the launchers dropin.c and particles.c name besides; neither is reached here */
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

#define SENT 777.0
#define SENT32 555.0f

/* one host-form call of n rays and P positions; which: bit 0 xyz, bit 1 xyz32, bit 2 count,
 * bit 3 hits */
static void run(int n, int P, int which, const char* what) {
    BlackHoleParams bh;
    initialize_black_hole_params(&bh, 1.0, 0.0, 0.0);
    AccretionDiskParams dk = {6.0, 20.0, 1.0, 1.0, 0.0, 0.0};
    SimulationConfig cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.time_step = 0.1;
    cfg.max_ray_distance = 100.0;
    cfg.max_integration_steps = 100;
    cfg.tolerance = 1e-6;
    const size_t N = (size_t)n, np = N * (size_t)P;
    /* exact-size allocations: ASan sees one element too many */
    Ray* rays = (Ray*)malloc(N * sizeof(Ray));
    Vector3D* xyz = (Vector3D*)malloc(np * sizeof(Vector3D));
    float* xyz32 = (float*)malloc(np * 3 * sizeof(float));
    int32_t* count = (int32_t*)malloc(N * sizeof(int32_t));
    int32_t* result = (int32_t*)malloc(N * sizeof(int32_t));
    int32_t* steps = (int32_t*)malloc(N * sizeof(int32_t));
    double* f8[8];
    for (int f = 0; f < 8; f++) f8[f] = (double*)malloc(N * sizeof(double));
    for (size_t i = 0; i < N; i++) {
        memset(&rays[i], 0, sizeof rays[i]);
        rays[i].origin.x = (double)i;
        rays[i].direction.z = -1.0;
        count[i] = -9;
    }
    for (size_t e = 0; e < np; e++) xyz[e].x = xyz[e].y = xyz[e].z = SENT;
    for (size_t e = 0; e < np * 3; e++) xyz32[e] = SENT32;
    bhrt_paths paths = {which & 1 ? xyz : NULL, which & 2 ? xyz32 : NULL, which & 4 ? count : NULL};
    bhrt_frame_soa hits;
    memset(&hits, 0, sizeof hits);
    hits.result = result;
    hits.steps = steps;
    hits.hit_x = f8[0];
    hits.hit_y = f8[1];
    hits.hit_z = f8[2];
    hits.distance = f8[3];
    hits.time_dilation = f8[4];
    hits.sky_x = f8[5];
    hits.sky_y = f8[6];
    hits.sky_z = f8[7];
    const long before = g_launches, traces_before = g_traces;
    const int rc = bhrt_trace_paths(rays, n, &bh, &dk, &cfg, INTEGRATOR_RK4, P, 1, &paths,
                                    which & 8 ? &hits : NULL);
    CHECK(rc == 0, "%s: rc %d (%s)", what, rc, bhrt_last_error());
    CHECK(g_launches == before + 1, "%s: %ld launches", what, g_launches - before);
    CHECK(g_traces == traces_before + (which & 8 ? 1 : 0), "%s: %ld hit launches", what,
          g_traces - traces_before);
    for (int i = 0; i < n && rc == 0; i++) {
        const int cnt = want_count(i, P);
        if (which & 4) CHECK(count[i] == cnt, "%s: count[%d] = %d, want %d", what, i, count[i], cnt);
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
        if (which & 8) {
            CHECK(result[i] == i % 5 && steps[i] == i + 3, "%s: hit %d", what, i);
            for (int f = 0; f < 8; f++)
                CHECK(f8[f][i] == enc_hit(f, i), "%s: hit field %d of ray %d", what, f, i);
        }
    }
    free(rays);
    free(xyz);
    free(xyz32);
    free(count);
    free(result);
    free(steps);
    for (int f = 0; f < 8; f++) free(f8[f]);
}

int main(void) {
    static const int combos[] = {1 | 4 | 8, 2 | 4, 1, 2 | 8, 4, 1 | 2 | 4 | 8};
    char what[96];
    /* readback forms (paths.c rows_back): the staged rectangle (the default for rows this
     * short), one copy per ray (a copy call priced at 0 bytes), one rectangle (every row full) */
    for (int form = 0; form < 3; form++) {
        if (form == 1) setenv("BHRT_PATHS_COPY_CALL_BYTES", "0", 1);
        else unsetenv("BHRT_PATHS_COPY_CALL_BYTES");
        g_full = form == 2;
        for (int k = 0; k < (int)(sizeof combos / sizeof *combos); k++)
            for (int n = 1; n <= 5; n += 4)
                for (int P = 1; P <= 7; P += 3) {
                    snprintf(what, sizeof what, "form %d outputs %d n %d P %d", form, combos[k], n, P);
                    run(n, P, combos[k], what);
                }
    }
    g_full = 0;
    bhrt_stats st;
    CHECK(bhrt_get_stats(&st, 1) == 0, "stats: %s", bhrt_last_error());
    CHECK((long)st.launches == g_launches + g_traces, "stats: %llu launches, %ld + %ld made",
          (unsigned long long)st.launches, g_launches, g_traces);
    CHECK(st.rays == (uint64_t)((g_launches + g_traces) / 2) * 6, "stats: %llu rays",
          (unsigned long long)st.rays);
    /* more launches than the control ring has slots: the claim counter is zero every time */
    for (int k = 0; k < 600; k++) run(1, 2, 1 | 4, "ring wrap");
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld launches)\n", g_launches);
    return 0;
}
