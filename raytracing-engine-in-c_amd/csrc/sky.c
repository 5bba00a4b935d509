/*
 * sky.c -- sky maps: an equirectangular environment texture on the device, bound to the calling
 * thread and looked up where a ray leaves the scene (the rule: include/bhrt_api.h "Sky maps").
 *
 * A map is one device allocation of width * height texels of 16 bytes -- r, g, b as float and a
 * pad -- so that a tap of the bilinear filter is one aligned load; both input formats are
 * converted on the host before the one upload. Binding copies the map's record (pointer, size,
 * the two texels-per-radian factors) into the host core's thread-level state (scene.c
 * bhrt_sky_bind); a launch with BHRT_FLAG_SKY carries it to the kernels in bhrt_kparams.sky.
 *
 * A file of its own (the Makefile's HOST_FEATURE): the files of HOST_CORE stay linkable without
 * the launcher named below (tests/fakehip).
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"

struct bhrt_sky {
    int device, format;
    bhrt_sky_k k;         /* the record a launch carries (chord is per launch: NULL here) */
    void* d_io;           /* bhrt_sky_lookup: device directions and colours of the host form */
    size_t cap_io;
};

static int check_device(const bhrt_sky* s) {
    const int dev = bhrt_current_device();
    if (dev != s->device) {
        bhrt_set_err("sky: made on device %d, the current device is %d", s->device, dev);
        return -1;
    }
    return 0;
}

int bhrt_sky_create(const void* texels, int W, int H, int format, bhrt_sky** sky) {
    if (!texels || !sky) {
        bhrt_set_err("sky: NULL argument");
        return -1;
    }
    if (W < 1 || H < 1) {
        bhrt_set_err("sky: invalid size %d x %d", W, H);
        return -1;
    }
    if ((long long)W * H > (1LL << 26)) {
        bhrt_set_err("sky: %d x %d texels are more than 2^26", W, H);
        return -1;
    }
    if (format != BHRT_SKY_RGB32F && format != BHRT_SKY_RGBA8) {
        bhrt_set_err("sky: unknown format %d", format);
        return -1;
    }
    const size_t n = (size_t)W * (size_t)H;
    if (format == BHRT_SKY_RGB32F) {
        const float* t = (const float*)texels;
        for (size_t i = 0; i < 3 * n; i++)
            if (!isfinite(t[i])) {
                bhrt_set_err("sky: texel (%zu, %zu) channel %zu is not finite", (i / 3) % (size_t)W,
                             (i / 3) / (size_t)W, i % 3);
                return -1;
            }
    }
    float* h = (float*)malloc(16 * n);
    bhrt_sky* s = (bhrt_sky*)calloc(1, sizeof *s);
    if (!h || !s) {
        free(h);
        free(s);
        bhrt_set_err("sky: out of memory");
        return -1;
    }
    if (format == BHRT_SKY_RGB32F) {
        const float* t = (const float*)texels;
        for (size_t i = 0; i < n; i++) {
            h[4 * i] = t[3 * i];
            h[4 * i + 1] = t[3 * i + 1];
            h[4 * i + 2] = t[3 * i + 2];
            h[4 * i + 3] = 1.0f;
        }
    } else {
        const unsigned char* t = (const unsigned char*)texels;
        for (size_t i = 0; i < n; i++) {
            h[4 * i] = (float)t[4 * i] / 255.0f;
            h[4 * i + 1] = (float)t[4 * i + 1] / 255.0f;
            h[4 * i + 2] = (float)t[4 * i + 2] / 255.0f;
            h[4 * i + 3] = 1.0f; /* alpha is ignored */
        }
    }
    const int dev = bhrt_current_device();
    void* d = NULL;
    hipError_t he = dev < 0 ? hipErrorNoDevice : hipMalloc(&d, 16 * n);
    if (he == hipSuccess) {
        /* complete on return: every stream may read the map afterwards */
        he = hipMemcpy(d, h, 16 * n, hipMemcpyHostToDevice);
        if (he != hipSuccess) (void)hipFree(d);
    }
    free(h);
    if (he != hipSuccess) {
        bhrt_set_err("sky: cannot place %zu bytes on the device: %s", 16 * n, hipGetErrorString(he));
        free(s);
        return -1;
    }
    s->device = dev;
    s->format = format;
    s->k.tex = d;
    s->k.w = W;
    s->k.h = H;
    s->k.sx = (double)W / (2.0 * BH_PI);
    s->k.sy = (double)H / BH_PI;
    *sky = s;
    return 0;
}

void bhrt_sky_destroy(bhrt_sky* s) {
    if (!s) return;
    if (bhrt_sky_bound() == s->k.tex) bhrt_sky_bind(NULL, -1);
    /* frames on any stream may still read the map: wait for the device, with it current */
    const int cur = bhrt_current_device();
    if (cur != s->device) (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    if (s->d_io) (void)hipFree(s->d_io);
    (void)hipFree((void*)s->k.tex);
    if (cur >= 0 && cur != s->device) (void)hipSetDevice(cur);
    free(s);
}

int bhrt_sky_info(const bhrt_sky* s, bhrt_sky_state* st) {
    if (!s || !st) {
        bhrt_set_err("sky: NULL argument");
        return -1;
    }
    st->width = s->k.w;
    st->height = s->k.h;
    st->format = s->format;
    st->device = s->device;
    return 0;
}

int bhrt_set_sky(const bhrt_sky* s) {
    if (s) bhrt_sky_bind(&s->k, s->device);
    else bhrt_sky_bind(NULL, -1);
    return 0;
}

typedef struct {
    const bhrt_sky* s;
    const double* dirs;
    int n;
    double* rgb;
} sky_call;

static int sky_body(devctx_t* c, hipStream_t st, const void* arg) {
    const sky_call* a = (const sky_call*)arg;
    (void)c;
    const int e = bhrt_launch_sky(&a->s->k, a->dirs, a->n, a->rgb, (void*)st);
    if (e != 0) {
        bhrt_set_err("sky lookup kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        return -1;
    }
    return 0;
}

static int check_lookup(const bhrt_sky* s, const double* dirs, int n, const double* rgb) {
    if (!s || !dirs || !rgb) {
        bhrt_set_err("sky: NULL argument");
        return -1;
    }
    if (n < 1) {
        bhrt_set_err("sky: n %d (>= 1)", n);
        return -1;
    }
    return check_device(s);
}

int bhrt_sky_lookup_device(const bhrt_sky* s, const double* d_dirs, int n, double* d_rgb,
                           void* stream) {
    if (check_lookup(s, d_dirs, n, d_rgb)) return -1;
    devctx_t* c = bhrt_ctx_get(s->device);
    if (!c) return -1;
    const sky_call a = {s, d_dirs, n, d_rgb};
    return bhrt_on_stream(c, (hipStream_t)stream, sky_body, &a);
}

int bhrt_sky_lookup(const bhrt_sky* s_in, const double* dirs, int n, double* rgb) {
    if (check_lookup(s_in, dirs, n, rgb)) return -1;
    bhrt_sky* s = (bhrt_sky*)s_in; /* (the host form's device arrays are kept with the object) */
    devctx_t* c = bhrt_ctx_get(s->device);
    if (!c || bhrt_ctx_streams(c)) return -1;
    const size_t bytes = align256(24 * (size_t)n);
    if (bhrt_ensure(&s->d_io, &s->cap_io, 2 * bytes, 0)) return -1;
    double* d_dirs = (double*)s->d_io;
    double* d_rgb = (double*)((char*)s->d_io + bytes);
    HIP_TRY(hipMemcpyAsync(d_dirs, dirs, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const sky_call a = {s, d_dirs, n, d_rgb};
    if (sky_body(c, c->stream, &a)) return -1;
    /* (the caller's array is pageable: a plain copy once the kernel is done, no async D2H) */
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(rgb, d_rgb, 24 * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}
