/* particles_resident_driver.c -- the host side of device-resident particle systems
 * (particles_resident.c over the HOST_CORE files) on SIMULATED devices (fake_hip.c), built by
 * tests/test_particles_resident_cpu.py under ASan+UBSan as a stand-alone program.
 *
 * The four launchers are stubs in host C that check every launch buffer against the simulated
 * device and do the kernels' work: the counting update is the oracle's update_particles
 * (oracle/oracle.c, linked in) followed by the per-workgroup counts, the count pass is the counts
 * alone, the scan is an exclusive scan with the total last, and the scatter places each active
 * particle at its workgroup's offset plus its rank within the workgroup. main() walks create /
 * update / extract (device and host form) / download / upload / destroy against a host copy stepped
 * by the oracle and the extract rule written out below, growth on upload, the refusals of a live
 * object -- a second device's among them --, and two objects on two simulated devices.
 * Test infrastructure only. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "bhrt_api.h"
#include "bhrt_kernel.h"

int fakehip_kind_of(const void* p, size_t n);
int fakehip_current_device(void);
void orc_update_particles(Particle* ps, int count, const BlackHoleParams* bh,
                          const SimulationConfig* cfg, int steps);

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

static BlackHoleParams g_bh;
static SimulationConfig g_cfg;
static int g_no_launch;   /* any launch now dies: a refused call must not reach a launcher */
static long g_updates, g_counts, g_scans, g_scatters;
static int g_want_steps;  /* the steps the next counting update must carry */
static const bhrt_particle_data* g_want_out; /* device form: the scatter writes these very arrays */

static int nblocks_of(int count) { return (count + 255) / 256; }

static void count_blocks(const Particle* d, int count, int* block_active) {
    for (int b = 0; b < nblocks_of(count); b++) {
        int c = 0;
        for (int i = 256 * b; i < count && i < 256 * (b + 1); i++) c += d[i].active != 0;
        block_active[b] = c;
    }
}

int bhrt_launch_particles_counted(Particle* d, int count, const bhrt_particle_k* k, int steps,
                                  int* block_active, void* stream, void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    if (g_no_launch) DIE("a refused call launched the update");
    if (count < 1 || steps < 1 || steps != g_want_steps) DIE("update of %d particles, %d steps", count, steps);
    on_device(d, (size_t)count * sizeof(Particle), "particles");
    on_device(block_active, (size_t)nblocks_of(count) * sizeof(int), "block_active");
    if (k->M != g_bh.mass || k->rs != g_bh.schwarzschild_radius || k->a != g_bh.spin * g_bh.mass ||
        k->r_plus != g_bh.r_plus || k->dt != g_cfg.time_step || k->spin0 != (g_bh.spin == 0.0))
        DIE("update launched with other constants than the call's");
    orc_update_particles(d, count, &g_bh, &g_cfg, steps);
    count_blocks(d, count, block_active);
    g_updates++;
    return 0;
}

int bhrt_launch_particles_count(const Particle* d, int count, int* block_active, void* stream) {
    (void)stream;
    if (g_no_launch) DIE("a refused call launched the count pass");
    if (count < 1) DIE("count pass of %d particles", count);
    on_device(d, (size_t)count * sizeof(Particle), "particles");
    on_device(block_active, (size_t)nblocks_of(count) * sizeof(int), "block_active");
    count_blocks(d, count, block_active);
    g_counts++;
    return 0;
}

int bhrt_launch_particles_scan(const int* block_active, int nblocks, int* offsets, void* stream,
                               void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    if (g_no_launch) DIE("a refused call launched the scan");
    if (nblocks < 1) DIE("scan of %d workgroups", nblocks);
    on_device(block_active, (size_t)nblocks * sizeof(int), "block_active");
    on_device(offsets, ((size_t)nblocks + 1) * sizeof(int), "offsets");
    int run = 0;
    for (int b = 0; b < nblocks; b++) {
        if (block_active[b] < 0 || block_active[b] > 256) DIE("block_active[%d] = %d", b, block_active[b]);
        offsets[b] = run;
        run += block_active[b];
    }
    offsets[nblocks] = run;
    g_scans++;
    return 0;
}

int bhrt_launch_particles_scatter(const Particle* d, int count, const int* offsets, int max_count,
                                  const bhrt_particle_data* out, void* stream, void* ev0, void* ev1) {
    (void)stream; (void)ev0; (void)ev1;
    if (g_no_launch) DIE("a refused call launched the scatter");
    const int nb = nblocks_of(count);
    on_device(d, (size_t)count * sizeof(Particle), "particles");
    on_device(offsets, ((size_t)nb + 1) * sizeof(int), "offsets");
    if (g_want_out && memcmp(out, g_want_out, sizeof *out) != 0)
        DIE("the scatter does not write the caller's device arrays");
    const size_t m = (size_t)(max_count < count ? max_count : count); /* what can be written */
    if (out->positions) on_device(out->positions, 24 * m, "positions");
    if (out->velocities) on_device(out->velocities, 24 * m, "velocities");
    if (out->types) on_device(out->types, 4 * m, "types");
    if (out->ids) on_device(out->ids, 4 * m, "ids");
    if (out->xyz32) on_device(out->xyz32, 12 * m, "xyz32");
    if (out->vel32) on_device(out->vel32, 12 * m, "vel32");
    if (out->count) on_device(out->count, 4, "count");
    for (int b = 0; b < nb; b++) {
        int rank = offsets[b];
        for (int i = 256 * b; i < count && i < 256 * (b + 1); i++) {
            if (!d[i].active) continue;
            const size_t r = (size_t)rank++;
            if (r >= (size_t)max_count) continue;
            const double x[3] = {d[i].position.x, d[i].position.y, d[i].position.z};
            const double v[3] = {d[i].velocity.x, d[i].velocity.y, d[i].velocity.z};
            for (int c = 0; c < 3; c++) {
                if (out->positions) out->positions[3 * r + c] = x[c];
                if (out->velocities) out->velocities[3 * r + c] = v[c];
                if (out->xyz32) out->xyz32[3 * r + c] = (float)x[c];
                if (out->vel32) out->vel32[3 * r + c] = (float)v[c];
            }
            if (out->types) out->types[r] = (int32_t)d[i].type;
            if (out->ids) out->ids[r] = d[i].id;
        }
        if (rank != offsets[b + 1]) DIE("workgroup %d: offsets do not match its active particles", b);
    }
    if (out->count) out->count[0] = offsets[nb] < max_count ? offsets[nb] : max_count;
    g_scatters++;
    return 0;
}

/* the launchers the HOST_CORE files name; none is reached here */
int bhrt_trace_untested(const bhrt_kparams* kp) { (void)kp; return 0; }
int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    (void)kp; (void)stream; (void)ev0; (void)ev1;
    return 100;
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
/* (fake_hip.c has no event destruction; bhrt_particles_destroy frees the timing events of
 * bhrt_particles_kernel_ms, which this driver never makes) */
hipError_t hipEventDestroy(hipEvent_t e) {
    free(e);
    return hipSuccess;
}

/* ---- host systems ---- */
static double urand(void) { return (double)rand() / RAND_MAX; }

/* n particles of mixed types, some just outside rs moving inward, every `off`-th inactive */
static void make_system(ParticleSystem* s, int n, int off) {
    if (particle_system_init(s, n + 8) != 0) DIE("particle_system_init");
    for (int i = 0; i < n; i++) {
        const double r = i % 5 == 2 ? g_bh.schwarzschild_radius + 0.01 + 0.3 * urand() : 6.0 + 30.0 * urand();
        const double phi = 6.28 * urand(), v = i % 5 == 2 ? -0.9 : sqrt(1.0 / r);
        const Vector3D pos = {r * cos(phi), r * sin(phi), 0.1 * (urand() - 0.5)};
        const Vector3D vel = i % 5 == 2 ? (Vector3D){v * cos(phi), v * sin(phi), 0.0}
                                        : (Vector3D){-v * sin(phi), v * cos(phi), 0.0};
        const ParticleType t = i % 5 == 2 ? PARTICLE_DISK : (ParticleType)(i % 4);
        if (add_particle(s, &pos, &vel, 1.0, t) < 0) DIE("add_particle");
        if (off > 0 && i % off == 0) s->particles[i].active = 0;
    }
}

typedef struct {
    double *positions, *velocities;
    int32_t *types, *ids;
    float *xyz32, *vel32;
    int count;
} rule_out;

/* the extract rule on a host array */
static rule_out rule(const Particle* p, int n, int max_count) {
    rule_out o;
    const size_t m = (size_t)max_count;
    o.positions = (double*)malloc(24 * m);
    o.velocities = (double*)malloc(24 * m);
    o.types = (int32_t*)malloc(4 * m);
    o.ids = (int32_t*)malloc(4 * m);
    o.xyz32 = (float*)malloc(12 * m);
    o.vel32 = (float*)malloc(12 * m);
    o.count = 0;
    for (int i = 0; i < n && o.count < max_count; i++) {
        if (!p[i].active) continue;
        const size_t r = (size_t)o.count++;
        const double x[3] = {p[i].position.x, p[i].position.y, p[i].position.z};
        const double v[3] = {p[i].velocity.x, p[i].velocity.y, p[i].velocity.z};
        for (int c = 0; c < 3; c++) {
            o.positions[3 * r + c] = x[c];
            o.velocities[3 * r + c] = v[c];
            o.xyz32[3 * r + c] = (float)x[c];
            o.vel32[3 * r + c] = (float)v[c];
        }
        o.types[r] = (int32_t)p[i].type;
        o.ids[r] = p[i].id;
    }
    return o;
}
static void rule_free(rule_out* o) {
    free(o->positions); free(o->velocities); free(o->types); free(o->ids); free(o->xyz32); free(o->vel32);
}

#define SENT 0x5A
/* `got` (max_count elements of `elem` bytes, sentinel-filled before the call) holds the rule's
 * `count` rows and the sentinel beyond */
static void check_field(const char* what, const char* field, const void* got, const void* want,
                        size_t elem, int count, int max_count) {
    CHECK(memcmp(got, want, elem * (size_t)count) == 0, "%s: %s differs from the rule", what, field);
    const unsigned char* g = (const unsigned char*)got;
    for (size_t i = elem * (size_t)count; i < elem * (size_t)max_count; i++)
        if (g[i] != SENT) {
            CHECK(0, "%s: %s written beyond the count at byte %zu", what, field, i);
            break;
        }
}

/* one extract of `ps` against the rule on `host`: device form (on `stream`), or host form; `mask`
 * picks the outputs (bit f = field f, bit 6 = count) */
static void extract_and_check(const char* what, bhrt_particles* ps, const Particle* host, int n,
                              int max_count, int mask, int host_form, hipStream_t stream) {
    const size_t m = (size_t)max_count;
    const size_t elem[7] = {24, 24, 4, 4, 12, 12, 4};
    void* arr[7];
    for (int f = 0; f < 7; f++) {
        arr[f] = NULL;
        if (!(mask >> f & 1)) continue;
        const size_t bytes = f == 6 ? 4 : elem[f] * m; /* exact sizes: ASan sees one byte too many */
        if (host_form) arr[f] = malloc(bytes);
        else if (hipMalloc(&arr[f], bytes) != hipSuccess) DIE("hipMalloc");
        memset(arr[f], SENT, bytes);
    }
    const bhrt_particle_data out = {(double*)arr[0], (double*)arr[1], (int32_t*)arr[2], (int32_t*)arr[3],
                                    (float*)arr[4], (float*)arr[5], (int32_t*)arr[6]};
    g_want_out = host_form ? NULL : &out;
    const int rc = host_form ? bhrt_particles_extract(ps, max_count, &out)
                             : bhrt_particles_extract_device(ps, max_count, &out, stream);
    g_want_out = NULL;
    CHECK(rc == 0, "%s: extract rc %d (%s)", what, rc, bhrt_last_error());
    rule_out w = rule(host, n, max_count);
    const void* want[6] = {w.positions, w.velocities, w.types, w.ids, w.xyz32, w.vel32};
    static const char* names[6] = {"positions", "velocities", "types", "ids", "xyz32", "vel32"};
    if (rc == 0) {
        for (int f = 0; f < 6; f++)
            if (arr[f]) check_field(what, names[f], arr[f], want[f], elem[f], w.count, max_count);
        if (arr[6]) CHECK(*(int32_t*)arr[6] == w.count, "%s: count %d, the rule's %d", what, *(int32_t*)arr[6], w.count);
    }
    rule_free(&w);
    for (int f = 0; f < 7; f++) {
        if (host_form) free(arr[f]);
        else (void)hipFree(arr[f]);
    }
}

static void same_particles(const char* what, const Particle* a, const Particle* b, int n) {
    for (int i = 0; i < n; i++)
        if (memcmp(&a[i], &b[i], sizeof(Particle)) != 0) {
            CHECK(0, "%s: particle %d differs", what, i);
            return;
        }
}

/* One object through the step sequence against a host copy; n particles, then an upload of n2 */
static void run(int n, int off, int n2, hipStream_t stream) {
    char what[96];
    snprintf(what, sizeof what, "n %d (every %d-th inactive), then %d%s", n, off, n2, stream ? "" : ", NULL stream");
    ParticleSystem sys, back;
    make_system(&sys, n, off);
    Particle* mirror = (Particle*)malloc((size_t)n * sizeof(Particle)); /* stepped by the oracle */
    memcpy(mirror, sys.particles, (size_t)n * sizeof(Particle));
    if (particle_system_init(&back, n) != 0) DIE("particle_system_init");
    back.count = n;
    memset(back.particles, 0, (size_t)n * sizeof(Particle));
    bhrt_particles* ps = NULL;
    const long counts0 = g_counts;
    if (bhrt_particles_create(&sys, &ps) != 0 || !ps) DIE("%s: create: %s", what, bhrt_last_error());
    CHECK(g_counts == counts0 + 1, "%s: create made %ld count passes", what, g_counts - counts0);
    const Particle* d_buf = NULL;
    int cnt = -1;
    CHECK(bhrt_particles_device_buffer(ps, &d_buf, &cnt) == 0 && cnt == n, "%s: device_buffer", what);
    on_device(d_buf, (size_t)n * sizeof(Particle), "resident array");
    bhrt_particles_state st;
    CHECK(bhrt_particles_info(ps, &st) == 0 && st.count == n && st.updates == 0 &&
              st.device == fakehip_current_device(), "%s: state after create", what);
    /* extract right after create: block_active comes from the count pass */
    extract_and_check(what, ps, mirror, n, n + 5, 0x7f, 0, stream);
    static const int seq[4] = {1, 1, 3, 10};
    int64_t updates = 0;
    for (int k = 0; k < 4; k++) {
        g_want_steps = seq[k];
        CHECK(bhrt_particles_update_device(ps, &g_bh, &g_cfg, seq[k], stream) == 0, "%s: update: %s", what, bhrt_last_error());
        orc_update_particles(mirror, n, &g_bh, &g_cfg, seq[k]);
        updates++;
        CHECK(bhrt_particles_update_device(ps, &g_bh, &g_cfg, 0, stream) == 0, "%s: steps 0", what);
        CHECK(bhrt_particles_info(ps, &st) == 0 && st.updates == updates, "%s: updates %lld", what, (long long)st.updates);
        CHECK(bhrt_particles_download(ps, &back) == 0, "%s: download: %s", what, bhrt_last_error());
        same_particles(what, back.particles, mirror, n);
        int active = 0;
        for (int i = 0; i < n; i++) active += mirror[i].active != 0;
        const int mc[6] = {1, active - 1, active, active + 1, n, n + 5};
        for (int j = 0; j < 6; j++) {
            if (mc[j] < 1) continue;
            extract_and_check(what, ps, mirror, n, mc[j], 0x7f, 0, stream);
            extract_and_check(what, ps, mirror, n, mc[j], 0x7f, 1, NULL);
        }
        extract_and_check(what, ps, mirror, n, n, 0x51, 0, stream); /* positions, xyz32, count */
        extract_and_check(what, ps, mirror, n, n, 0x08, 1, NULL);   /* ids alone, host form */
        extract_and_check(what, ps, mirror, n, n, 0x40, 0, stream); /* the count alone */
    }
    CHECK(back.capacity == n && back.next_id == 1, "%s: download touched the system's other members", what);
    /* the refusals of a live object: nothing launched, nothing written, the state as it was */
    g_no_launch = 1;
    double sentinel[3] = {7.0, 7.0, 7.0};
    const bhrt_particle_data some = {sentinel, NULL, NULL, NULL, NULL, NULL, NULL};
    const bhrt_particle_data none = {NULL, NULL, NULL, NULL, NULL, NULL, NULL};
    ParticleSystem empty = sys, nullp = sys, other = back;
    empty.count = 0;
    nullp.particles = NULL;
    other.count = n - 1;
    CHECK(bhrt_particles_update_device(ps, NULL, &g_cfg, 1, stream) == -1, "%s: NULL blackhole", what);
    CHECK(bhrt_particles_update_device(ps, &g_bh, NULL, 1, stream) == -1, "%s: NULL config", what);
    CHECK(bhrt_particles_update_device(ps, &g_bh, &g_cfg, -1, stream) == -1 && strstr(bhrt_last_error(), "steps"), "%s: steps -1", what);
    CHECK(bhrt_particles_extract_device(ps, 0, &some, stream) == -1 && strstr(bhrt_last_error(), "max_count"), "%s: max_count 0", what);
    CHECK(bhrt_particles_extract_device(ps, 4, NULL, stream) == -1, "%s: NULL output struct", what);
    CHECK(bhrt_particles_extract_device(ps, 4, &none, stream) == -1, "%s: seven NULL outputs", what);
    CHECK(bhrt_particles_extract(ps, 0, &some) == -1 && bhrt_particles_extract(ps, 4, NULL) == -1 &&
              bhrt_particles_extract(ps, 4, &none) == -1, "%s: host extract refusals", what);
    CHECK(bhrt_particles_upload(ps, NULL) == -1 && bhrt_particles_upload(ps, &empty) == -1 &&
              bhrt_particles_upload(ps, &nullp) == -1, "%s: upload refusals", what);
    CHECK(bhrt_particles_download(ps, NULL) == -1, "%s: download NULL", what);
    if (n > 1) CHECK(bhrt_particles_download(ps, &other) == -1 && strstr(bhrt_last_error(), "resident"), "%s: download count mismatch", what);
    CHECK(sentinel[0] == 7.0 && sentinel[1] == 7.0 && sentinel[2] == 7.0, "%s: a refused call wrote", what);
    bhrt_particles_state st1;
    CHECK(bhrt_particles_info(ps, &st1) == 0 && memcmp(&st, &st1, sizeof st) == 0, "%s: a refused call moved the state", what);
    g_no_launch = 0;
    /* upload after a host-side change: some particles removed, n2 - n added (growth, or fewer) */
    ParticleSystem sys2;
    make_system(&sys2, n2, 3);
    for (int i = 0; i < n2; i += 4) (void)remove_particle(&sys2, sys2.particles[i].id);
    CHECK(bhrt_particles_upload(ps, &sys2) == 0, "%s: upload: %s", what, bhrt_last_error());
    CHECK(bhrt_particles_info(ps, &st) == 0 && st.count == n2 && st.updates == updates, "%s: state after upload", what);
    extract_and_check(what, ps, sys2.particles, n2, n2, 0x7f, 0, stream);
    extract_and_check(what, ps, sys2.particles, n2, n2 + 5, 0x7f, 1, NULL);
    g_want_steps = 2;
    CHECK(bhrt_particles_update_device(ps, &g_bh, &g_cfg, 2, stream) == 0, "%s: update after upload", what);
    orc_update_particles(sys2.particles, n2, &g_bh, &g_cfg, 2);
    extract_and_check(what, ps, sys2.particles, n2, n2, 0x7f, 1, NULL);
    (void)bhrt_particles_device_buffer(ps, &d_buf, NULL);
    bhrt_particles_destroy(ps);
    CHECK(fakehip_kind_of(d_buf, 1) != fakehip_current_device(), "%s: destroy left the resident array allocated", what);
    particle_system_cleanup(&sys);
    particle_system_cleanup(&sys2);
    particle_system_cleanup(&back);
    free(mirror);
}

int main(void) {
    initialize_black_hole_params(&g_bh, 1.0, 0.0, 0.0);
    memset(&g_cfg, 0, sizeof g_cfg);
    g_cfg.time_step = 0.05;
    g_cfg.max_ray_distance = 100.0;
    g_cfg.max_integration_steps = 100;
    g_cfg.tolerance = 1e-6;
    srand(11);
    hipStream_t st;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) DIE("stream");
    run(1, 0, 3, st);
    run(255, 2, 257, st);
    run(256, 0, 64, NULL);
    run(257, 3, 2000, st);   /* growth on upload */
    run(1000, 1, 700, NULL); /* none active */
    /* NULL arguments: refused before anything else, the handle untouched */
    ParticleSystem sys;
    make_system(&sys, 10, 0);
    bhrt_particles* h = (bhrt_particles*)&g_fail;
    ParticleSystem empty = sys, nullp = sys;
    empty.count = 0;
    nullp.particles = NULL;
    g_no_launch = 1;
    CHECK(bhrt_particles_create(NULL, &h) == -1 && bhrt_particles_create(&empty, &h) == -1 &&
              bhrt_particles_create(&nullp, &h) == -1 && bhrt_particles_create(&sys, NULL) == -1,
          "create accepted a bad argument");
    CHECK(h == (bhrt_particles*)&g_fail, "a refused create wrote the handle");
    bhrt_particles_state s7 = {7, 7, 7};
    double d7 = 7.0;
    const bhrt_particle_data some = {&d7, NULL, NULL, NULL, NULL, NULL, NULL};
    CHECK(bhrt_particles_upload(NULL, &sys) == -1 && bhrt_particles_update_device(NULL, &g_bh, &g_cfg, 1, st) == -1 &&
              bhrt_particles_extract_device(NULL, 1, &some, st) == -1 && bhrt_particles_extract(NULL, 1, &some) == -1 &&
              bhrt_particles_download(NULL, &sys) == -1 && bhrt_particles_device_buffer(NULL, NULL, NULL) == -1 &&
              bhrt_particles_info(NULL, &s7) == -1, "a NULL object accepted");
    CHECK(strstr(bhrt_last_error(), "NULL object") != NULL, "message: %s", bhrt_last_error());
    CHECK(s7.count == 7 && s7.updates == 7 && d7 == 7.0, "a refused call wrote");
    bhrt_particles_destroy(NULL);
    g_no_launch = 0;
    /* create / destroy: every allocation freed again */
    for (int i = 0; i < 100; i++) {
        bhrt_particles* a = NULL;
        const Particle* buf = NULL;
        if (bhrt_particles_create(&sys, &a) != 0) DIE("create %d: %s", i, bhrt_last_error());
        (void)bhrt_particles_device_buffer(a, &buf, NULL);
        bhrt_particles_destroy(a);
        CHECK(fakehip_kind_of(buf, 1) != fakehip_current_device(), "create/destroy %d leaked", i);
    }
    /* an object is bound to its device; two objects on two devices are independent */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 1) {
        bhrt_particles *a = NULL, *b = NULL;
        ParticleSystem sysb;
        make_system(&sysb, 300, 2);
        Particle* ma = (Particle*)malloc(10 * sizeof(Particle));
        Particle* mb = (Particle*)malloc(300 * sizeof(Particle));
        memcpy(ma, sys.particles, 10 * sizeof(Particle));
        memcpy(mb, sysb.particles, 300 * sizeof(Particle));
        if (bhrt_particles_create(&sys, &a) != 0) DIE("create: %s", bhrt_last_error());
        if (hipSetDevice(1) != hipSuccess) DIE("hipSetDevice(1)");
        hipStream_t st1;
        if (hipStreamCreateWithFlags(&st1, hipStreamNonBlocking) != hipSuccess) DIE("stream");
        if (bhrt_particles_create(&sysb, &b) != 0) DIE("create on device 1: %s", bhrt_last_error());
        g_no_launch = 1;
        CHECK(bhrt_particles_update_device(a, &g_bh, &g_cfg, 1, st1) == -1 && strstr(bhrt_last_error(), "current device") != NULL,
              "update on another device: %s", bhrt_last_error());
        CHECK(bhrt_particles_extract_device(a, 1, &some, st1) == -1 && bhrt_particles_extract(a, 1, &some) == -1 &&
                  bhrt_particles_upload(a, &sys) == -1 && bhrt_particles_download(a, &sys) == -1,
              "an object used from a second device");
        CHECK(strstr(bhrt_last_error(), "current device") != NULL && d7 == 7.0, "message: %s", bhrt_last_error());
        g_no_launch = 0;
        for (int k = 0; k < 3; k++) { /* interleaved: b on device 1, a on device 0 */
            g_want_steps = 2;
            CHECK(bhrt_particles_update_device(b, &g_bh, &g_cfg, 2, st1) == 0, "b update: %s", bhrt_last_error());
            orc_update_particles(mb, 300, &g_bh, &g_cfg, 2);
            if (hipSetDevice(0) != hipSuccess) DIE("hipSetDevice(0)");
            g_want_steps = 1;
            CHECK(bhrt_particles_update_device(a, &g_bh, &g_cfg, 1, st) == 0, "a update: %s", bhrt_last_error());
            orc_update_particles(ma, 10, &g_bh, &g_cfg, 1);
            extract_and_check("object a on device 0", a, ma, 10, 10, 0x7f, k & 1, st);
            if (hipSetDevice(1) != hipSuccess) DIE("hipSetDevice(1)");
            extract_and_check("object b on device 1", b, mb, 300, 305, 0x7f, k & 1, st1);
        }
        bhrt_particles_state sa;
        CHECK(bhrt_particles_info(a, &sa) == 0 && sa.updates == 3 && sa.device == 0, "a's state");
        bhrt_particles_destroy(b);
        if (hipSetDevice(0) != hipSuccess) DIE("hipSetDevice(0)");
        bhrt_particles_destroy(a);
        particle_system_cleanup(&sysb);
        free(ma);
        free(mb);
    } else {
        CHECK(0, "the driver needs two simulated devices (FAKEHIP_DEVICES=2)");
    }
    particle_system_cleanup(&sys);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("all checks passed (%ld updates, %ld count passes, %ld scans, %ld scatters)\n", g_updates,
           g_counts, g_scans, g_scatters);
    return 0;
}
