/* adaptive_driver.c -- the host side of adaptive supersampled frames (adaptive.c, over
 * supersample.c's argument check and the HOST_CORE files) on a SIMULATED device (fake_hip.c),
 * built by tests/test_adaptive_cpu.py under ASan+UBSan as a stand-alone program.
 *
 * The launchers are stubs that check every launch buffer against the simulated device and fill
 * the device arrays from host code: the ray kernels write an encoding of (pass, ray, axis) into
 * the directions, the trace an encoding of (pass, ray, channel) into the sample planes after
 * checking the directions it was given, the edge kernel a KNOWN edge count with the list and the
 * slots of a fixed pattern (none, every third pixel, all), slots handed out in descending order.
 * The resolve stub then checks that every base plane still holds its encoding -- i.e. that the
 * base planes survived the second launch's allocation -- and the extra planes theirs, and adds
 * sample 0 of each pass into the outputs, which main() checks pixel by pixel with the call's
 * bhrt_adaptive_info and the statistics. Whole images go through the host form, shards through
 * the device form on a stream and on the NULL stream. Test infrastructure only. */
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

/* ---- the frame under test ---- */
static int g_W, g_H, g_B, g_M, g_pattern; /* pattern 0: no edge, 1: every third pixel, 2: all */
static bhrt_rows g_rows;
static int g_n, g_next, g_E;              /* owned pixels, ext pixels, edge pixels */
static int g_ext_rows[256], g_ext_of[256], g_own_rows[256];
static int g_pass;                        /* trace launches of this frame so far */
static long g_traces, g_trace_rays;

static int owned(int y) {
    return g_rows.num_shards <= 1 || (y / g_rows.row_block) % g_rows.num_shards == g_rows.shard;
}
static int is_edge(int p) { return g_pattern == 2 || (g_pattern == 1 && p % 3 == 0); }
static int slot_of(int p) { /* descending: the first edge pixel gets the last slot */
    int rank = 0;
    for (int i = 0; i < p; i++) rank += is_edge(i);
    return is_edge(p) ? g_E - 1 - rank : -1;
}
static int image_pixel(int p) { return g_own_rows[p / g_W] * g_W + p % g_W; }
static double enc_dir(int pass, long ray, int c) { return pass * 1e7 + ray * 4.0 + c + 0.125; }
static double enc_col(int pass, long ray, int c) { return pass * 1e7 + ray * 4.0 + c + 0.5; }

static void plan(int W, int H, bhrt_rows rows, int B, int M, int pattern) {
    g_W = W, g_H = H, g_rows = rows, g_B = B, g_M = M, g_pattern = pattern;
    int e = 0, o = 0;
    for (int y = 0; y < H; y++) {
        const int near = owned(y) || (y > 0 && owned(y - 1)) || (y + 1 < H && owned(y + 1));
        g_ext_of[y] = near ? e : -1;
        if (near) g_ext_rows[e++] = y;
        if (owned(y)) g_own_rows[o++] = y;
    }
    g_n = o * W;
    g_next = e * W;
    g_E = 0;
    for (int p = 0; p < g_n; p++) g_E += is_edge(p);
    g_pass = 0;
}

/* ---- the stub launchers ---- */
int bhrt_launch_ad_rays(const bhrt_ad_rays_k* k, void* stream) {
    (void)stream;
    const int extra = k->pixels != NULL;
    const int want_n = extra ? g_E : g_next;
    if (k->n != want_n) DIE("ray launch of %d rays, want %d", k->n, want_n);
    if (g_pass != extra) DIE("ray launch of pass %d after %d trace launches", extra, g_pass);
    if (k->cam.width != g_W || k->cam.height != g_H || k->cam.rows.num_shards > 1)
        DIE("ray launch without the whole image's camera");
    on_device(k->dirs + k->first * 3, 24 * (size_t)k->n, "directions");
    if (extra) {
        on_device(k->pixels, 4 * (size_t)k->n, "edge list");
        for (int p = 0; p < g_n; p++)
            if (is_edge(p) && k->pixels[slot_of(p)] != image_pixel(p))
                DIE("edge list slot %d holds %d, want %d", slot_of(p), k->pixels[slot_of(p)],
                    image_pixel(p));
    } else if (g_rows.num_shards > 1) {
        on_device(k->rows, 4 * (size_t)(g_next / g_W), "ext rows");
        for (int e = 0; e < g_next / g_W; e++)
            if (k->rows[e] != g_ext_rows[e]) DIE("ext row %d is %d, want %d", e, k->rows[e], g_ext_rows[e]);
    } else if (k->rows) {
        DIE("a whole image has no row table");
    }
    for (long r = 0; r < k->n; r++)
        for (int c = 0; c < 3; c++) k->dirs[(k->first + r) * 3 + c] = enc_dir(extra, k->first + r, c);
    return 0;
}

int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    const int pass = g_pass;
    const size_t n = (size_t)kp->n;
    const size_t want = pass == 0 ? (size_t)g_next * g_B : (size_t)g_E * (g_M - g_B);
    if (pass > 1 || n != want) DIE("trace launch %d of %zu rays, want %zu", pass, n, want);
    if (!kp->rays_shared || kp->rays || kp->dir_stride != 3 || kp->src != BHRT_SRC_RAYS)
        DIE("not a shared-origin launch of packed directions");
    on_device(kp->dirs, 24 * n, "directions");
    on_device(kp->init, (size_t)(BHRT_INIT_FIELDS + 1) * 8 * n, "launch scratch");
    on_device(kp->ctl, 8 * 8, "control block");
    on_device(kp->out.rgb_r, 8 * n, "r plane");
    on_device(kp->out.rgb_g, 8 * n, "g plane");
    on_device(kp->out.rgb_b, 8 * n, "b plane");
    if (pass == 0) on_device(kp->out.result, 4 * n, "class plane");
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++)
            if (kp->dirs[i * 3 + c] != enc_dir(pass, (long)i, c))
                DIE("pass %d ray %zu direction %d is %g", pass, i, c, kp->dirs[i * 3 + c]);
    memset(kp->init, 0x5a, (size_t)(BHRT_INIT_FIELDS + 1) * 8 * n); /* (the kernel's own use) */
    for (size_t i = 0; i < n; i++) {
        kp->out.rgb_r[i] = enc_col(pass, (long)i, 0);
        kp->out.rgb_g[i] = enc_col(pass, (long)i, 1);
        kp->out.rgb_b[i] = enc_col(pass, (long)i, 2);
        if (kp->out.result) kp->out.result[i] = (int)(i % 5);
    }
    kp->ctl[1] += n;
    g_pass++;
    g_traces++;
    g_trace_rays += (long)n;
    return 0;
}

int bhrt_launch_ad_edges(const bhrt_ad_edges_k* k, void* stream) {
    (void)stream;
    if (g_pass != 1) DIE("edge launch after %d trace launches", g_pass);
    if (k->n != g_n || k->width != g_W || k->height != g_H || k->next != g_next ||
        k->base != g_B || k->max != g_M)
        DIE("edge launch: n %d next %ld B %d M %d", k->n, k->next, k->base, k->max);
    on_device(k->r, 8 * (size_t)g_next * g_B, "r planes");
    on_device(k->slot, 4 * (size_t)g_n, "slots");
    on_device(k->list, 4 * (size_t)g_n, "edge list");
    on_device(k->count, 8, "edge counter");
    if (*k->count != 0) DIE("edge counter is %llu at launch", *k->count);
    if (g_rows.num_shards > 1) {
        on_device(k->ext_of, 4 * (size_t)g_H, "ext_of");
        for (int y = 0; y < g_H; y++)
            if (k->ext_of[y] != g_ext_of[y]) DIE("ext_of[%d] is %d, want %d", y, k->ext_of[y], g_ext_of[y]);
        if (k->rows.row_block != g_rows.row_block || k->rows.shard != g_rows.shard ||
            k->rows.num_shards != g_rows.num_shards)
            DIE("edge launch without the shard");
    } else if (k->ext_of) {
        DIE("a whole image has no row table");
    }
    for (int p = 0; p < g_n; p++) {
        k->slot[p] = slot_of(p);
        if (is_edge(p)) k->list[slot_of(p)] = image_pixel(p);
    }
    *k->count = (unsigned long long)g_E;
    return 0;
}

static void* g_samples_seen;
int bhrt_launch_ad_resolve(const bhrt_ad_resolve_k* k, void* stream) {
    (void)stream;
    const int extra = g_E > 0 && g_M > g_B;
    if (g_pass != 1 + extra) DIE("resolve after %d trace launches, want %d", g_pass, 1 + extra);
    if (k->n != g_n || k->next != g_next || k->nedge != g_E || k->base != g_B || k->max != g_M)
        DIE("resolve launch: n %d next %ld E %ld", k->n, k->next, k->nedge);
    const double* base[3] = {k->r, k->g, k->b};
    const double* xtr[3] = {k->xr, k->xg, k->xb};
    on_device(k->result, 4 * (size_t)g_next * g_B, "class planes");
    on_device(k->slot, 4 * (size_t)g_n, "slots");
    for (int c = 0; c < 3; c++) {
        /* the base planes, written before the second launch's scratch was asked for */
        on_device(base[c], 8 * (size_t)g_next * g_B, "base plane");
        for (long i = 0; i < (long)g_next * g_B; i++)
            if (base[c][i] != enc_col(0, i, c)) DIE("base plane %d lost ray %ld: %g", c, i, base[c][i]);
        if (!extra) continue;
        on_device(xtr[c], 8 * (size_t)g_E * (g_M - g_B), "extra plane");
        for (long i = 0; i < (long)g_E * (g_M - g_B); i++)
            if (xtr[c][i] != enc_col(1, i, c)) DIE("extra plane %d lost ray %ld: %g", c, i, xtr[c][i]);
    }
    for (int i = 0; i < g_next * g_B; i++)
        if (k->result[i] != i % 5) DIE("class plane lost ray %d", i);
    for (int p = 0; p < g_n; p++) {
        if (k->slot[p] != slot_of(p)) DIE("slot of pixel %d lost", p);
        const int pix = image_pixel(p);
        const long q = (long)g_ext_of[pix / g_W] * g_W + pix % g_W;
        double v[3];
        for (int c = 0; c < 3; c++)
            v[c] = base[c][q] + (k->slot[p] >= 0 && extra ? xtr[c][k->slot[p]] : 0.0);
        if (k->out.rgb_r) {
            on_device(k->out.rgb_r + p, 8, "rgb_r");
            k->out.rgb_r[p] = v[0], k->out.rgb_g[p] = v[1], k->out.rgb_b[p] = v[2];
        }
        if (k->out.rgba8) {
            on_device(k->out.rgba8 + 4 * p, 4, "rgba8");
            k->out.rgba8[4 * p] = (uint8_t)(p % 251);
        }
        if (k->out.result) k->out.result[p] = k->result[q];
        if (k->samples) {
            on_device(k->samples + p, 4, "samples");
            k->samples[p] = k->slot[p] >= 0 ? g_M : g_B;
        }
    }
    g_samples_seen = k->samples;
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

/* ---- one frame ---- */
static long g_want_rays;

static void check_frame(const char* what, const double* r, const double* g, const double* b,
                        const int32_t* result, const int32_t* samples, const uint8_t* rgba8,
                        const bhrt_adaptive_info* info) {
    const int extra = g_E > 0 && g_M > g_B;
    for (int p = 0; p < g_n; p++) {
        const int pix = image_pixel(p), slot = slot_of(p);
        const long q = (long)g_ext_of[pix / g_W] * g_W + pix % g_W;
        const double* got[3] = {r, g, b};
        for (int c = 0; c < 3 && r; c++) {
            const double want = enc_col(0, q, c) + (slot >= 0 && extra ? enc_col(1, slot, c) : 0.0);
            CHECK(got[c][p] == want, "%s: pixel %d channel %d = %g, want %g", what, p, c, got[c][p], want);
        }
        if (result) CHECK(result[p] == (int)(q % 5), "%s: class of pixel %d", what, p);
        if (samples)
            CHECK(samples[p] == (slot >= 0 ? g_M : g_B), "%s: samples[%d] = %d", what, p, samples[p]);
        if (rgba8) CHECK(rgba8[4 * p] == (uint8_t)(p % 251), "%s: rgba8 of pixel %d", what, p);
    }
    const long halo = g_next - g_n;
    const long rays = (long)g_next * g_B + (long)g_E * (g_M - g_B);
    CHECK(info->pixels == g_n && info->edge_pixels == g_E && info->halo_pixels == halo &&
              info->sample_rays == rays,
          "%s: info %lld %lld %lld %lld, want %d %d %ld %ld", what, (long long)info->pixels,
          (long long)info->edge_pixels, (long long)info->sample_rays, (long long)info->halo_pixels,
          g_n, g_E, rays, halo);
    CHECK(g_pass == 1 + extra, "%s: %d trace launches", what, g_pass);
    g_want_rays += rays;
}

static void scene(BlackHoleParams* bh, AccretionDiskParams* dk, SimulationConfig* cfg,
                  bhrt_camera* cam, SupersamplingParams* ss, AdaptiveSamplingParams* as) {
    initialize_black_hole_params(bh, 1.0, 0.0, 0.0);
    const AccretionDiskParams d = {6.0, 20.0, 1.0, 1.0, 0.0, 0.0};
    *dk = d;
    memset(cfg, 0, sizeof *cfg);
    cfg->time_step = 0.1;
    cfg->max_ray_distance = 100.0;
    cfg->max_integration_steps = 100;
    cfg->tolerance = 1e-6;
    memset(cam, 0, sizeof *cam);
    cam->position.z = 30.0;
    cam->position.y = 3.0;
    cam->direction.z = -1.0;
    cam->up.y = 1.0;
    cam->fov_deg = 40.0;
    memset(ss, 0, sizeof *ss);
    ss->samples_per_pixel = 4;
    ss->jitter_method = JITTER_REGULAR_GRID;
    ss->jitter_strength = 1.0;
    memset(as, 0, sizeof *as);
    as->enable_adaptive = 1;
    as->min_samples = g_B;
    as->max_samples = g_M;
    as->edge_threshold = 0.1;
}

/* a whole image through the host form; fields: bit 0 rgb, 1 result, 2 samples, 3 rgba8 */
static void run_host(int W, int H, int B, int M, int pattern, int fields) {
    char what[96];
    snprintf(what, sizeof what, "host %dx%d %d->%d pattern %d fields %d", W, H, B, M, pattern, fields);
    const bhrt_rows whole = {0, 0, 1};
    plan(W, H, whole, B, M, pattern);
    BlackHoleParams bh; AccretionDiskParams dk; SimulationConfig cfg; bhrt_camera cam;
    SupersamplingParams ss; AdaptiveSamplingParams as;
    scene(&bh, &dk, &cfg, &cam, &ss, &as);
    const size_t n = (size_t)g_n; /* exact-size allocations: ASan sees one element too many */
    double* r = (double*)malloc(8 * n); double* g = (double*)malloc(8 * n);
    double* b = (double*)malloc(8 * n);
    int32_t* result = (int32_t*)malloc(4 * n); int32_t* samples = (int32_t*)malloc(4 * n);
    uint8_t* rgba8 = (uint8_t*)malloc(4 * n);
    bhrt_frame_soa out;
    memset(&out, 0, sizeof out);
    if (fields & 1) out.rgb_r = r, out.rgb_g = g, out.rgb_b = b;
    if (fields & 2) out.result = result;
    if (fields & 8) out.rgba8 = rgba8;
    bhrt_adaptive_info info;
    const int rc = bhrt_render_frame_adaptive(&bh, &dk, &cfg, &cam, W, H, INTEGRATOR_RK4, 0, &ss,
                                              &as, &out, fields & 4 ? samples : NULL, &info);
    CHECK(rc == 0, "%s: rc %d (%s)", what, rc, bhrt_last_error());
    if (rc == 0) {
        CHECK((g_samples_seen != NULL) == ((fields & 4) != 0), "%s: samples array", what);
        check_frame(what, fields & 1 ? r : NULL, g, b, fields & 2 ? result : NULL,
                    fields & 4 ? samples : NULL, fields & 8 ? rgba8 : NULL, &info);
    }
    free(r); free(g); free(b); free(result); free(samples); free(rgba8);
}

/* every shard of a sharded image through the device form, on `stream` */
static void run_shards(int W, int H, int row_block, int shards, int B, int M, int pattern,
                       hipStream_t stream) {
    for (int s = 0; s < shards; s++) {
        char what[96];
        snprintf(what, sizeof what, "shard %d of (%d, %d) %dx%d %d->%d pattern %d%s", s, row_block,
                 shards, W, H, B, M, pattern, stream ? "" : " NULL stream");
        const bhrt_rows rows = {row_block, s, shards};
        plan(W, H, rows, B, M, pattern);
        CHECK(bhrt_shard_rows(H, &rows) * W == g_n, "%s: %d owned pixels", what, g_n);
        BlackHoleParams bh; AccretionDiskParams dk; SimulationConfig cfg; bhrt_camera cam;
        SupersamplingParams ss; AdaptiveSamplingParams as;
        scene(&bh, &dk, &cfg, &cam, &ss, &as);
        const size_t n = (size_t)(g_n ? g_n : 1);
        bhrt_frame_soa out;
        memset(&out, 0, sizeof out);
        int32_t* d_samples = NULL;
        if (hipMalloc((void**)&out.rgb_r, 8 * n) || hipMalloc((void**)&out.rgb_g, 8 * n) ||
            hipMalloc((void**)&out.rgb_b, 8 * n) || hipMalloc((void**)&out.result, 4 * n) ||
            hipMalloc((void**)&d_samples, 4 * n))
            DIE("hipMalloc failed");
        bhrt_adaptive_info info;
        const int rc = bhrt_render_frame_adaptive_device(&bh, &dk, &cfg, &cam, W, H, &rows,
                                                         INTEGRATOR_RK4, 0, &ss, &as, &out,
                                                         d_samples, &info, stream);
        CHECK(rc == 0, "%s: rc %d (%s)", what, rc, bhrt_last_error());
        if (rc == 0 && g_n > 0)
            check_frame(what, out.rgb_r, out.rgb_g, out.rgb_b, out.result, d_samples, NULL, &info);
        if (rc == 0 && g_n > 0 && H > 1) CHECK(info.halo_pixels > 0, "%s: no halo", what);
        (void)hipFree(out.rgb_r); (void)hipFree(out.rgb_g); (void)hipFree(out.rgb_b);
        (void)hipFree(out.result); (void)hipFree(d_samples);
    }
}

int main(void) {
    /* edge counts 0, some and all; B = 1, M = 4 with every pixel an edge makes the second
     * launch's scratch request larger than anything asked for before: a new allocation */
    for (int pattern = 0; pattern < 3; pattern++) {
        run_host(7, 5, 1, 4, pattern, 1 | 2 | 4 | 8);
        run_host(7, 5, 2, 3, pattern, 1);
        run_host(1, 1, 1, 2, pattern, 4 | 8);
    }
    run_host(5, 3, 2, 2, 2, 1 | 4);       /* M == B: edge pixels without a second launch */
    run_host(13, 11, 1, 4, 2, 1 | 2 | 4); /* grows every block again */
    hipStream_t st;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) DIE("stream");
    for (int pattern = 0; pattern < 3; pattern++) {
        run_shards(6, 16, 3, 2, 1, 4, pattern, st);
        run_shards(6, 9, 1, 2, 2, 4, pattern, st);
        run_shards(5, 18, 2, 3, 1, 3, pattern, NULL);
        run_shards(4, 40, 8, 3, 1, 4, pattern, st);  /* shards of 16, 16 and 8 rows */
        run_shards(3, 5, 4, 3, 1, 2, pattern, st);   /* the third shard owns no row */
    }
    run_shards(9, 31, 2, 2, 1, 4, 2, st);            /* grows the blocks mid-sequence */
    bhrt_stats stt;
    CHECK(bhrt_get_stats(&stt, 1) == 0, "stats: %s", bhrt_last_error());
    CHECK((long)stt.launches == g_traces, "stats: %llu launches, %ld made",
          (unsigned long long)stt.launches, g_traces);
    CHECK((long)stt.rays == g_trace_rays && g_trace_rays == g_want_rays,
          "stats: %llu rays, %ld traced, %ld in the frames' info", (unsigned long long)stt.rays,
          g_trace_rays, g_want_rays);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld trace launches, %ld rays)\n", g_traces, g_trace_rays);
    return 0;
}
