/*
 * kerr_particles.c -- physical particles: a device-resident particle system advanced along true
 * timelike geodesics of Kerr in coordinate time (the rule: include/bhrt_api.h "Physical
 * particles"; the kernel: kerr.hip k_kerr_particles). An opt-in update beside the parity update
 * of particles_resident.c, on the same object: nothing here is reached by any other entry point.
 *
 * The call is its argument checks -- every refusal is decided before any HIP call -- and one launch
 * on the caller's stream under the stream rule, with no host wait, as
 * bhrt_particles_update_device's. Like that update it takes no control block of the context's ring
 * and adds nothing to bhrt_stats.
 *
 * A file of its own (the Makefile's HOST_FEATURE): particles_resident.c and the files of HOST_CORE
 * stay linkable without the launcher named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <math.h>
#include <string.h>

#include "bhrt_host.h"
#include "particles_resident.h"

typedef struct {
    bhrt_particles* p;
    bhrt_kerr_particles_k k;
    int steps;
} kp_call;

static int kp_body(devctx_t* c, hipStream_t st, const void* arg) {
    const kp_call* u = (const kp_call*)arg;
    (void)c;
    const int e = bhrt_launch_kerr_particles(u->p->d_buf, u->p->count, &u->k, u->steps,
                                             u->p->d_blocks, (void*)st, NULL, NULL);
    if (e != 0) {
        bhrt_set_err("kerr particle kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    return 0;
}

int bhrt_particles_kerr_update_device(bhrt_particles* p, const BlackHoleParams* bh,
                                      const SimulationConfig* cfg, int steps,
                                      const bhrt_kerr_particles_params* params,
                                      const bhrt_kerr_particles_diag* diag, void* stream) {
    if (check_object(p)) return -1;
    if (!bh || !cfg) {
        bhrt_set_err("particles: NULL blackhole or config");
        return -1;
    }
    if (steps < 0) {
        bhrt_set_err("particles: steps %d (>= 0)", steps);
        return -1;
    }
    kp_call u;
    memset(&u, 0, sizeof u);
    /* the scene's checks and constants; of the config the time step alone is read */
    const SimulationConfig dt_only = {.time_step = cfg->time_step};
    if (bhrt_kerr_scene(bh, NULL, &dt_only, &u.k.k)) return -1;
    if (!params) {
        bhrt_set_err("kerr particles: NULL params");
        return -1;
    }
    if (params->substeps < 1 || params->substeps > 64) {
        bhrt_set_err("kerr particles: substeps %d (1..64)", params->substeps);
        return -1;
    }
    if (check_device(p)) return -1;
    if (steps == 0) return 0;
    u.k.k.a = bh->spin * bh->mass; /* forward in time: +(spin * mass), a^2 and r+ as they are */
    u.k.substeps = params->substeps;
    if (diag) {
        u.k.k.h_residual = diag->h_residual;
        u.k.k.lz_drift = diag->lz_drift;
        u.k.status = diag->status;
        u.k.substeps_out = diag->substeps;
    }
    u.p = p;
    u.steps = steps;
    devctx_t* c = bhrt_ctx_get(p->device);
    if (!c) return -1;
    if (bhrt_on_stream(c, (hipStream_t)stream, kp_body, &u)) return -1;
    p->updates++;
    used_on(p, c, (hipStream_t)stream);
    return 0;
}
