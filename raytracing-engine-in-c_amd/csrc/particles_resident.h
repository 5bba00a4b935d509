/*
 * particles_resident.h -- the device-resident particle object as its two updates see it:
 * particles_resident.c (the object, the parity update, the extracts) and kerr_particles.c (the
 * physical update). Private to those two files.
 */
#ifndef BHRT_PARTICLES_RESIDENT_H
#define BHRT_PARTICLES_RESIDENT_H

#include "bhrt_host.h"

struct bhrt_particles {
    int device, count;
    int64_t updates;
    Particle* d_buf;      /* the resident array */
    size_t cap;           /* particles */
    int* d_blocks;        /* block_active [cap_blocks], then offsets [cap_blocks + 1] */
    size_t cap_blocks;
    void* d_out;          /* bhrt_particles_extract: device outputs of the host form */
    size_t cap_out;
    void* h_out;          /* ... and their pinned staging */
    size_t cap_hout;
    hipEvent_t ev[10];    /* bhrt_particles_kernel_ms */
    int have_ev;
    hipStream_t last;     /* the stream of the last update or device extract */
    int used;
};

static inline int check_object(const bhrt_particles* p) {
    if (!p) {
        bhrt_set_err("particles: NULL object");
        return -1;
    }
    return 0;
}

static inline int check_device(const bhrt_particles* p) {
    const int dev = bhrt_current_device();
    if (dev != p->device) {
        bhrt_set_err("particles: made on device %d, the current device is %d", p->device, dev);
        return -1;
    }
    return 0;
}

/* an update or a device extract was queued on `stream` (NULL: the context's own) */
static inline void used_on(bhrt_particles* p, devctx_t* c, hipStream_t stream) {
    p->last = stream ? stream : c->stream;
    p->used = 1;
}

#endif
