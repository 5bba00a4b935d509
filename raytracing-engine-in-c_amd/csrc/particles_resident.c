/*
 * particles_resident.c -- device-resident particle systems: the visualizer's physics tick
 * (bh_update_particles, then bh_get_particle_data, renderer.cpp:926-951) on an object that keeps
 * the Particle array on the GPU (the rule: include/bhrt_api.h).
 *
 * The object owns, on its device: the Particle array (grown with slack on upload), block_active
 * -- per 256-lane workgroup of the update kernel, the number of its particles that are active --
 * and the scanned offsets. The invariant: block_active is current after every create, upload and
 * update (create and upload establish it with one count-only pass, the counting update kernel keeps
 * it), so an extract is the scan of nblocks ints and the scatter, and never reads the 152-byte
 * structs to find a flag. Update and device extract run on the caller's stream with no host wait;
 * the calls that wait (upload, the host extract, download, destroy) first wait for the stream of
 * the last of those. The host extract goes through device arrays of the object's own and pinned
 * staging: caller memory is never page-locked.
 *
 * A file of its own (the Makefile's HOST_FEATURE): the files of HOST_CORE stay linkable without
 * the four launchers named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"
#include "particles_resident.h" /* the object, check_object, check_device, used_on */

#define BHRT_PARTICLES_ONE_COPY ((size_t)1 << 20) /* bytes: the host extract's single D2H */

static int nblocks_of(int count) { return (count + 255) / 256; }
static int* offsets_of(const bhrt_particles* p) { return p->d_blocks + p->cap_blocks; }

static void fill_k(bhrt_particle_k* k, const BlackHoleParams* bh, const SimulationConfig* cfg) {
    k->M = bh->mass; /* as bhrt_update_particles_steps fills it (particles.c) */
    k->rs = bh->schwarzschild_radius;
    k->a = bh->spin * bh->mass;
    k->r_plus = bh->r_plus;
    k->dt = cfg->time_step;
    k->spin0 = bh->spin == 0.0;
}

/* ---- the refusals, all before any HIP call but the current device's query ---- */
static int check_system(const ParticleSystem* s) {
    if (!s) {
        bhrt_set_err("particles: NULL system");
        return -1;
    }
    if (s->count < 1 || !s->particles) {
        bhrt_set_err("particles: empty system (count %d, particles %s)", s->count,
                     s->particles ? "set" : "NULL");
        return -1;
    }
    return 0;
}

static int check_out(int max_count, const bhrt_particle_data* out) {
    if (max_count < 1) {
        bhrt_set_err("particles: max_count %d (>= 1)", max_count);
        return -1;
    }
    if (!out) {
        bhrt_set_err("particles: NULL output struct");
        return -1;
    }
    if (!out->positions && !out->velocities && !out->types && !out->ids && !out->xyz32 &&
        !out->vel32 && !out->count) {
        bhrt_set_err("particles: every output pointer is NULL");
        return -1;
    }
    return 0;
}

static int wait_last(bhrt_particles* p) {
    if (p->used) HIP_TRY(hipStreamSynchronize(p->last));
    p->used = 0;
    return 0;
}

/* system->particles into the resident array (grown if need be) and block_active of it, complete on
 * return; the object's count changes only when all of it succeeded */
static int load_system(bhrt_particles* p, const ParticleSystem* s) {
    devctx_t* c = bhrt_ctx_get(p->device);
    if (!c || bhrt_ctx_streams(c)) return -1;
    if (wait_last(p)) return -1;
    const size_t n = (size_t)s->count;
    if (p->cap < n) {
        const size_t cap = n + n / 4 + 256, blocks = (cap + 255) / 256;
        Particle* d = NULL;
        int* b = NULL;
        HIP_TRY(hipMalloc((void**)&d, cap * sizeof(Particle)));
        const hipError_t he = hipMalloc((void**)&b, (2 * blocks + 1) * sizeof(int));
        if (he != hipSuccess) {
            bhrt_set_err("particles: allocation failed: %s", hipGetErrorString(he));
            (void)hipFree(d);
            return -1;
        }
        if (p->d_buf) (void)hipFree(p->d_buf);
        if (p->d_blocks) (void)hipFree(p->d_blocks);
        p->d_buf = d;
        p->d_blocks = b;
        p->cap = cap;
        p->cap_blocks = blocks;
    }
    HIP_TRY(hipMemcpyAsync(p->d_buf, s->particles, n * sizeof(Particle), hipMemcpyHostToDevice,
                           c->stream));
    const int e = bhrt_launch_particles_count(p->d_buf, s->count, p->d_blocks, (void*)c->stream);
    if (e != 0) {
        bhrt_set_err("particle count kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    p->count = s->count;
    return 0;
}

int bhrt_particles_create(const ParticleSystem* system, bhrt_particles** ps) {
    if (!ps) {
        bhrt_set_err("particles: NULL object");
        return -1;
    }
    if (check_system(system)) return -1;
    const int dev = bhrt_current_device();
    if (dev < 0) {
        bhrt_set_err("particles: no current device");
        return -1;
    }
    bhrt_particles* p = (bhrt_particles*)calloc(1, sizeof *p);
    if (!p) {
        bhrt_set_err("particles: out of memory");
        return -1;
    }
    p->device = dev;
    if (load_system(p, system)) {
        bhrt_particles_destroy(p);
        return -1;
    }
    *ps = p;
    return 0;
}

int bhrt_particles_upload(bhrt_particles* p, const ParticleSystem* system) {
    if (check_object(p) || check_system(system) || check_device(p)) return -1;
    return load_system(p, system);
}

void bhrt_particles_destroy(bhrt_particles* p) {
    if (!p) return;
    if (p->used) (void)hipStreamSynchronize(p->last);
    if (p->have_ev)
        for (int i = 0; i < 10; i++) (void)hipEventDestroy(p->ev[i]);
    if (p->h_out) (void)hipHostFree(p->h_out);
    if (p->d_out) (void)hipFree(p->d_out);
    if (p->d_blocks) (void)hipFree(p->d_blocks);
    if (p->d_buf) (void)hipFree(p->d_buf);
    free(p);
}

int bhrt_particles_info(const bhrt_particles* p, bhrt_particles_state* state) {
    if (check_object(p)) return -1;
    if (!state) {
        bhrt_set_err("particles: NULL state");
        return -1;
    }
    state->count = p->count;
    state->device = p->device;
    state->updates = p->updates;
    return 0;
}

int bhrt_particles_device_buffer(const bhrt_particles* p, const Particle** device_particles,
                                 int* count) {
    if (check_object(p)) return -1;
    if (device_particles) *device_particles = p->d_buf;
    if (count) *count = p->count;
    return 0;
}

/* ---- update ---- */
typedef struct {
    bhrt_particles* p;
    bhrt_particle_k k;
    int steps;
} up_call;

static int up_body(devctx_t* c, hipStream_t st, const void* arg) {
    const up_call* u = (const up_call*)arg;
    (void)c;
    const int e = bhrt_launch_particles_counted(u->p->d_buf, u->p->count, &u->k, u->steps,
                                                u->p->d_blocks, (void*)st, NULL, NULL);
    if (e != 0) {
        bhrt_set_err("particle kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    return 0;
}

int bhrt_particles_update_device(bhrt_particles* p, const BlackHoleParams* bh,
                                 const SimulationConfig* cfg, int steps, void* stream) {
    if (check_object(p)) return -1;
    if (!bh || !cfg) {
        bhrt_set_err("particles: NULL blackhole or config");
        return -1;
    }
    if (steps < 0) {
        bhrt_set_err("particles: steps %d (>= 0)", steps);
        return -1;
    }
    if (check_device(p)) return -1;
    if (steps == 0) return 0;
    devctx_t* c = bhrt_ctx_get(p->device);
    if (!c) return -1;
    up_call u;
    u.p = p;
    u.steps = steps;
    fill_k(&u.k, bh, cfg);
    if (bhrt_on_stream(c, (hipStream_t)stream, up_body, &u)) return -1;
    p->updates++;
    used_on(p, c, (hipStream_t)stream);
    return 0;
}

/* ---- extract ---- */
typedef struct {
    bhrt_particles* p;
    int max_count;
    const bhrt_particle_data* out;
    hipEvent_t* ev; /* NULL, or four events around the scan and the scatter */
} ex_call;

static int ex_body(devctx_t* c, hipStream_t st, const void* arg) {
    const ex_call* x = (const ex_call*)arg;
    const bhrt_particles* p = x->p;
    (void)c;
    int e = bhrt_launch_particles_scan(p->d_blocks, nblocks_of(p->count), offsets_of(p), (void*)st,
                                       x->ev ? (void*)x->ev[0] : NULL,
                                       x->ev ? (void*)x->ev[1] : NULL);
    if (e == 0)
        e = bhrt_launch_particles_scatter(p->d_buf, p->count, offsets_of(p), x->max_count, x->out,
                                          (void*)st, x->ev ? (void*)x->ev[2] : NULL,
                                          x->ev ? (void*)x->ev[3] : NULL);
    if (e != 0) {
        bhrt_set_err("particle extract kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    return 0;
}

int bhrt_particles_extract_device(bhrt_particles* p, int max_count, const bhrt_particle_data* out,
                                  void* stream) {
    if (check_object(p) || check_out(max_count, out) || check_device(p)) return -1;
    devctx_t* c = bhrt_ctx_get(p->device);
    if (!c) return -1;
    const ex_call x = {p, max_count, out, NULL};
    if (bhrt_on_stream(c, (hipStream_t)stream, ex_body, &x)) return -1;
    used_on(p, c, (hipStream_t)stream);
    return 0;
}

int bhrt_particles_extract(bhrt_particles* p, int max_count, const bhrt_particle_data* out) {
    if (check_object(p) || check_out(max_count, out) || check_device(p)) return -1;
    devctx_t* c = bhrt_ctx_get(p->device);
    if (!c || bhrt_ctx_streams(c)) return -1;
    if (wait_last(p)) return -1;
    /* device arrays for the caller's, kept with the object: at most m elements are written */
    const size_t m = (size_t)(max_count < p->count ? max_count : p->count);
    const size_t b24 = align256(24 * m), b12 = align256(12 * m), b4 = align256(4 * m);
    const size_t bytes = 2 * b24 + 2 * b4 + 2 * b12 + 256;
    if (bhrt_ensure(&p->d_out, &p->cap_out, bytes, 0) ||
        bhrt_ensure(&p->h_out, &p->cap_hout, bytes, 1))
        return -1;
    const size_t off[7] = {0, b24, 2 * b24, 2 * b24 + b4, 2 * b24 + 2 * b4, 2 * b24 + 2 * b4 + b12,
                           2 * b24 + 2 * b4 + 2 * b12};
    const size_t elem[6] = {24, 24, 4, 4, 12, 12};
    void* const host[6] = {out->positions, out->velocities, out->types, out->ids, out->xyz32,
                           out->vel32};
    char* const d = (char*)p->d_out;
    char* const h = (char*)p->h_out;
    bhrt_particle_data dev;
    memset(&dev, 0, sizeof dev);
    if (out->positions) dev.positions = (double*)(d + off[0]);
    if (out->velocities) dev.velocities = (double*)(d + off[1]);
    if (out->types) dev.types = (int32_t*)(d + off[2]);
    if (out->ids) dev.ids = (int32_t*)(d + off[3]);
    if (out->xyz32) dev.xyz32 = (float*)(d + off[4]);
    if (out->vel32) dev.vel32 = (float*)(d + off[5]);
    dev.count = (int32_t*)(d + off[6]);
    const ex_call x = {p, max_count, &dev, NULL};
    if (ex_body(c, c->stream, &x)) return -1;
    /* a small system in one copy and one wait; a large one the count first, so that only the
     * elements written cross the bus */
    const int whole = off[6] + 4 <= BHRT_PARTICLES_ONE_COPY;
    HIP_TRY(hipMemcpyAsync(whole ? h : h + off[6], whole ? d : d + off[6], whole ? off[6] + 4 : 4,
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int32_t written;
    memcpy(&written, h + off[6], 4);
    if (written < 0 || (size_t)written > m) {
        bhrt_set_err("particles: the device wrote a count of %d (at most %zu)", (int)written, m);
        return -1;
    }
    if (whole) {
        for (int f = 0; f < 6; f++)
            if (host[f]) memcpy(host[f], h + off[f], elem[f] * (size_t)written);
    } else if (written > 0) {
        for (int f = 0; f < 6; f++)
            if (host[f])
                HIP_TRY(hipMemcpyAsync(h + off[f], d + off[f], elem[f] * (size_t)written,
                                       hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int f = 0; f < 6; f++)
            if (host[f]) memcpy(host[f], h + off[f], elem[f] * (size_t)written);
    }
    if (out->count) out->count[0] = written;
    return 0;
}

int bhrt_particles_download(bhrt_particles* p, ParticleSystem* system) {
    if (check_object(p) || check_system(system)) return -1;
    if (system->count != p->count) {
        bhrt_set_err("particles: download into a system of %d particles, %d are resident",
                     system->count, p->count);
        return -1;
    }
    if (check_device(p)) return -1;
    if (wait_last(p)) return -1;
    /* a plain synchronous copy: caller memory is never page-locked */
    HIP_TRY(hipMemcpy(system->particles, p->d_buf, (size_t)p->count * sizeof(Particle),
                      hipMemcpyDeviceToHost));
    return 0;
}

int bhrt_particles_kernel_ms(bhrt_particles* p, const BlackHoleParams* bh,
                             const SimulationConfig* cfg, int max_count,
                             const bhrt_particle_data* out, double ms[5]) {
    if (check_object(p)) return -1;
    if (!bh || !cfg || !ms) {
        bhrt_set_err("particles: NULL blackhole, config or ms");
        return -1;
    }
    if (check_out(max_count, out) || check_device(p)) return -1;
    devctx_t* c = bhrt_ctx_get(p->device);
    if (!c || bhrt_ctx_streams(c)) return -1;
    if (wait_last(p)) return -1;
    if (!p->have_ev) {
        for (int i = 0; i < 10; i++) HIP_TRY(hipEventCreate(&p->ev[i]));
        p->have_ev = 1;
    }
    bhrt_particle_k k;
    fill_k(&k, bh, cfg);
    /* each kernel twice and the SECOND timed, so that both timed launches follow an update pass
     * over the array: at 4.19 M particles an update behind another update's 637 MB of writes takes
     * 0.267 ms, one behind an extract's reads or an upload 0.233 ms, whichever kernel it is
     * (profiles/particles_resident/kernel_times.txt) */
    int e = bhrt_launch_particles(p->d_buf, p->count, &k, 1, (void*)c->stream, NULL, NULL);
    if (e == 0)
        e = bhrt_launch_particles(p->d_buf, p->count, &k, 1, (void*)c->stream, (void*)p->ev[0],
                                  (void*)p->ev[1]);
    for (int r = 0; r < 2 && e == 0; r++) /* (restores block_active, which the plain kernel left) */
        e = bhrt_launch_particles_counted(p->d_buf, p->count, &k, 1, p->d_blocks, (void*)c->stream,
                                          r ? (void*)p->ev[2] : NULL, r ? (void*)p->ev[3] : NULL);
    if (e != 0) {
        bhrt_set_err("particle kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    p->updates += 4;
    const ex_call x = {p, max_count, out, &p->ev[4]};
    if (ex_body(c, c->stream, &x)) return -1;
    /* the count pass of create and upload, for comparison (it rewrites the same counts) */
    HIP_TRY(hipEventRecord(p->ev[8], c->stream));
    e = bhrt_launch_particles_count(p->d_buf, p->count, p->d_blocks, (void*)c->stream);
    if (e != 0) {
        bhrt_set_err("particle count kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    HIP_TRY(hipEventRecord(p->ev[9], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 5; i++) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, p->ev[2 * i], p->ev[2 * i + 1]));
        ms[i] = t;
    }
    return 0;
}
