// frames.hip -- the elementwise frame passes of the geodesic ray tracer, one lane per item, no
// integration: the sky lookup of given directions, the ray directions and resolves of supersampled
// and adaptive frames, and the blend and edge passes of temporal accumulation, with their
// launchers. The camera mapping (camera_dir, div_floor) and the colour stores (bhrt_colour.h) are
// bhrt_trace_core.h's, so a pass's bits are the trace path's. The host sides are sky.c,
// supersample.c, adaptive.c and temporal.c.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bhrt_kernel.h"

#pragma clang fp contract(fast)

namespace {

#include "bhrt_trace_core.h"

// bhrt_sky_lookup_device: sky_lookup of n packed directions, one lane each
__global__ __launch_bounds__(256) void k_sky_lookup(const bhrt_sky_k sk, const double* dirs, int n,
                                                    double* rgb) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double r, g, b;
    sky_lookup(sk, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], r, g, b);
    rgb[3 * i] = r;
    rgb[3 * i + 1] = g;
    rgb[3 * i + 2] = b;
}

// Supersampled frames (bhrt_kernel.h bhrt_ss_rays_k): the directions of one sample's rays, one
// lane per pixel. camera_dir itself on the argument block's camera, which carries the sample's
// offset in place of the camera's: the row shard mapping and the direction arithmetic are the
// camera path's own, and so are the directions' bits (test_gpu_supersample.py).
__global__ __launch_bounds__(256) void k_ss_rays(const bhrt_ss_rays_k a) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n) return;  // (the last workgroup's partial wave)
    double dx, dy, dz;
    camera_dir(a.cam, (int)p, dx, dy, dz);
    double* d = a.dirs + ((size_t)a.sample * (size_t)a.n + (size_t)p) * 3;
    d[0] = dx;
    d[1] = dy;
    d[2] = dz;
}

// trace_pixel's average (raytracer.c:1131-1164), one lane per pixel: the S sample colours added
// in sample order from 0.0 and divided by S, as IEEE operations (no contraction), then the
// outputs exactly as store_colour converts them; the class is sample 0's. Sample plane s is
// contiguous, so every load and store of a wave is one contiguous run.
__global__ __launch_bounds__(256) void k_ss_resolve(const bhrt_ss_resolve_k a) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n) return;  // (the last workgroup's partial wave)
    double r = 0.0, g = 0.0, b = 0.0;
    for (int s = 0; s < a.samples; s++) {
        const size_t i = (size_t)s * (size_t)a.n + (size_t)p;
        r = r + a.r[i];
        g = g + a.g[i];
        b = b + a.b[i];
    }
    const double ns = (double)a.samples;
    r = r / ns;
    g = g / ns;
    b = b / ns;
    store_colour(a.out, (int)p, r, g, b);
    if (a.out.result) a.out.result[p] = a.result[p];
}

// Adaptive supersampled frames (bhrt_kernel.h bhrt_ad_rays_k; the rule: bhrt_api.h). The
// directions of one sample's rays, one lane per ray, addressed by IMAGE pixel: camera_dir on the
// whole image's camera, read in place with the sample's offset in it as k_ss_rays reads its own,
// so the directions are the supersampled frame's bit for bit (test_gpu_adaptive.py).
__global__ __launch_bounds__(256) void k_ad_rays(const bhrt_ad_rays_k a) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;  // (the last workgroup's partial wave)
    int pix = (int)r;
    if (a.pixels) {
        pix = a.pixels[r];
    } else if (a.rows) {
        const int W = a.cam.width;
        const int e = div_floor((int)r, W, a.cam.inv_width);
        pix = a.rows[e] * W + ((int)r - e * W);
    }
    double dx, dy, dz;
    camera_dir(a.cam, pix, dx, dy, dz);
    double* d = a.dirs + ((size_t)a.first + (size_t)r) * 3;
    d[0] = dx;
    d[1] = dy;
    d[2] = dz;
}

// shard pixel p's image column and row (camera_dir's own mapping)
__device__ __forceinline__ void ad_pixel(int p, int W, const bhrt_rows& rows, double inv_width,
                                         double inv_block, int& px, int& py) {
    const int j = div_floor(p, W, inv_width);
    px = p - j * W;
    py = j;
    if (rows.num_shards > 1) {
        const int B = rows.row_block;
        const int jb = div_floor(j, B, inv_block);
        py = (jb * rows.num_shards + rows.shard) * B + (j - jb * B);
    }
}

// step 1 of the rule: the base colour of ext pixel q
__device__ __forceinline__ void ad_base(const double* pr, const double* pg, const double* pb,
                                        size_t next, int B, size_t q, double& r, double& g,
                                        double& b) {
#pragma clang fp contract(off)
    r = g = b = 0.0;
    for (int s = 0; s < B; s++) {
        const size_t i = (size_t)s * next + q;
        r = r + pr[i];
        g = g + pg[i];
        b = b + pb[i];
    }
    const double nb = (double)B;
    r = r / nb;
    g = g / nb;
    b = b / nb;
}

// Steps 2 to 4, one lane per owned pixel: the edge value over the 4-neighbourhood in the image,
// the decision, and the edge pixels compacted into a list -- per wave one ballot, the lane's
// rank among the set bits below it, and ONE returning atomic on the counter. The slot order
// follows the waves' arrival and differs from run to run; nothing downstream depends on it (a
// pixel finds its extra samples through its own slot).
__global__ __launch_bounds__(256) void k_ad_edges(const bhrt_ad_edges_k a) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = p < a.n;  // (no early exit: the whole wave takes part in the ballot)
    bool edge = false;
    int pix = 0;
    if (live) {
        const int W = a.width;
        int px, py;
        ad_pixel((int)p, W, a.rows, a.inv_width, a.inv_block, px, py);
        pix = py * W + px;
        const size_t next = (size_t)a.next;
        const int e = a.ext_of ? a.ext_of[py] : py;
        double r, g, b;
        ad_base(a.r, a.g, a.b, next, a.base, (size_t)e * W + px, r, g, b);
        double gmax = 0.0;
        for (int k = 0; k < 4; k++) {
            const int qx = px + (k == 0 ? -1 : (k == 1 ? 1 : 0));
            const int qy = py + (k == 2 ? -1 : (k == 3 ? 1 : 0));
            if (qx < 0 || qx >= W || qy < 0 || qy >= a.height) continue;
            const int qe = a.ext_of ? a.ext_of[qy] : qy;
            if (qe < 0) continue;  // (never: a shard's ext rows hold its rows' vertical neighbours)
            double qr, qg, qb;
            ad_base(a.r, a.g, a.b, next, a.base, (size_t)qe * W + qx, qr, qg, qb);
            const double d = (fabs(r - qr) + fabs(g - qg) + fabs(b - qb)) / 3.0;
            if (d > gmax) gmax = d;  // (false for a NaN d)
        }
        edge = gmax > a.threshold;  // (false for a NaN threshold)
    }
    const unsigned long long m = __ballot(edge);
    int slot = -1;
    if (m) {  // (wave-uniform)
        const int lane = (int)(threadIdx.x & 63u), leader = __ffsll((long long)m) - 1;
        int first = 0;
        if (lane == leader) first = (int)atomicAdd(a.count, (unsigned long long)__popcll(m));
        first = __shfl(first, leader);
        if (edge) {
            slot = first + __popcll(m & ((1ull << lane) - 1ull));
            a.list[slot] = pix;
        }
    }
    if (live) a.slot[p] = slot;
}

// Step 5, one lane per owned pixel: the sequential sum over the base planes continued over the
// pixel's extra samples (through its slot), divided by S(p); the outputs as store_colour
// converts them, sample 0's class, and S(p).
__global__ __launch_bounds__(256) void k_ad_resolve(const bhrt_ad_resolve_k a) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n) return;  // (the last workgroup's partial wave)
    const int W = a.width;
    int px, py;
    ad_pixel((int)p, W, a.rows, a.inv_width, a.inv_block, px, py);
    const int e = a.ext_of ? a.ext_of[py] : py;
    const size_t q = (size_t)e * W + px, next = (size_t)a.next;
    double r = 0.0, g = 0.0, b = 0.0;
    for (int s = 0; s < a.base; s++) {
        const size_t i = (size_t)s * next + q;
        r = r + a.r[i];
        g = g + a.g[i];
        b = b + a.b[i];
    }
    const int slot = a.slot[p];
    int S = a.base;
    if (slot >= 0) {
        S = a.max;
        for (int s = 0; s < a.max - a.base; s++) {
            const size_t i = (size_t)s * (size_t)a.nedge + (size_t)slot;
            r = r + a.xr[i];
            g = g + a.xg[i];
            b = b + a.xb[i];
        }
    }
    const double ns = (double)S;
    r = r / ns;
    g = g / ns;
    b = b / ns;
    store_colour(a.out, (int)p, r, g, b);
    if (a.out.result) a.out.result[p] = a.result[q];
    if (a.samples) a.samples[p] = S;
}

// Temporal accumulation (bhrt_kernel.h bhrt_ta_blend_k; the rule: bhrt_api.h). All float32, no
// contraction, as the reference's x86 build evaluates accumulateFrame, detectEdges and
// finalizeAccumulatedFrame (renderer.cpp:1759-1877).
struct ta_f3 {  // 12 bytes, 4-byte aligned: one dwordx3 load or store
    float x, y, z;
};

// Step 6 of one channel, the ONE place that decides the gamma: std::min / std::max as the
// reference calls them (NaN -> 1.0f, -0.0f -> 0.0f), then the DOUBLE pow of the float operands
// rounded to float -- within a double ulp of the exact power, so the float is the correctly
// rounded one but for ties no image meets, where powf's 1-ulp result would move the truncation
// at every byte boundary it straddles -- times 255.0f, truncated toward zero.
__device__ __forceinline__ unsigned ta_gamma_u8(float c) {
#pragma clang fp contract(off)
    const float m = (c < 1.0f) ? c : 1.0f;
    const float k = (0.0f < m) ? m : 0.0f;
    const float g = (float)pow((double)k, (double)(1.0f / 2.2f));
    return (unsigned)(int)(g * 255.0f) & 0xffu;
}

// Steps 1 to 3 and 6, one lane per pixel: a 16-byte (the trace's rgba32f) or 12-byte (a caller's
// frame) load of the new colour, a 12-byte load and store of acc, the optional 12-byte copy and
// one packed 4-byte rgba8 store. Step 1's zeroing is a select, not a fill.
__global__ __launch_bounds__(256) void k_ta_blend(const bhrt_ta_blend_k a) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * 256 + (size_t)threadIdx.x;
    if (p >= (size_t)a.n) return;  // (the last workgroup's partial wave)
    ta_f3 f;
    if (a.stride == 4) {
        const float4 v = reinterpret_cast<const float4*>(a.frame)[p];
        f.x = v.x;
        f.y = v.y;
        f.z = v.z;
    } else {
        f = reinterpret_cast<const ta_f3*>(a.frame)[p];
    }
    ta_f3* acc = reinterpret_cast<ta_f3*>(a.acc) + p;
    ta_f3 c = {0.0f, 0.0f, 0.0f};
    if (!a.zero) c = *acc;
    c.x = c.x * a.w + f.x * a.alpha;
    c.y = c.y * a.w + f.y * a.alpha;
    c.z = c.z * a.w + f.z * a.alpha;
    *acc = c;
    if (a.rgb) reinterpret_cast<ta_f3*>(a.rgb)[p] = c;
    if (a.rgba8)
        reinterpret_cast<unsigned*>(a.rgba8)[p] =
            ta_gamma_u8(c.x) | (ta_gamma_u8(c.y) << 8) | (ta_gamma_u8(c.z) << 16) | 0xff000000u;
}

// Step 5, one lane per pixel of a whole image, launched behind k_ta_blend on the same stream: the
// stencil reads the UPDATED acc of the four neighbours (mostly from the L2 the blend just wrote).
// Border pixels never touch edge[] (it stays 0 from creation) and report 0.
__global__ __launch_bounds__(256) void k_ta_edges(const bhrt_ta_edges_k a) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * 256 + (size_t)threadIdx.x;
    if (p >= (size_t)a.n) return;  // (the last workgroup's partial wave)
    const unsigned W = (unsigned)a.width, H = (unsigned)a.height;
    const unsigned y = (unsigned)p / W, x = (unsigned)p - y * W;  // (n <= INT_MAX)
    float e = 0.0f;
    if (x >= 1u && x + 1u < W && y >= 1u && y + 1u < H) {
        const ta_f3* A = reinterpret_cast<const ta_f3*>(a.acc);
        const ta_f3 c = A[p];
        const size_t q[4] = {p - (size_t)W, p + (size_t)W, p - 1, p + 1};
        float g = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const ta_f3 v = A[q[k]];
            float d = 0.0f;
            d = d + fabsf(c.x - v.x);
            d = d + fabsf(c.y - v.y);
            d = d + fabsf(c.z - v.z);
            d = d / 3.0f;
            if (d > g) g = d;  // (false for a NaN d)
        }
        const float dec = a.edge[p] - a.decay;
        e = (g > a.threshold) ? 1.0f : ((0.0f < dec) ? dec : 0.0f);  // (NaN threshold: decay)
        a.edge[p] = e;
    }
    if (a.out) a.out[p] = e;
}

// One lane per item with a tail guard in the kernel: (n + 255) / 256 workgroups of 256 lanes on
// the stream (n <= INT_MAX, so the workgroup count fits an unsigned).
template <class Args>
int launch_items(void (*kernel)(const Args), const Args& a, long n, void* stream) {
    kernel<<<(unsigned)((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int bhrt_launch_sky(const bhrt_sky_k* sky, const double* d_dirs, int n, double* d_rgb,
                               void* stream) {
    if (n <= 0) return 0;
    k_sky_lookup<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(*sky, d_dirs, n,
                                                                               d_rgb);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_ss_rays(const bhrt_ss_rays_k* k, void* stream) {
    if (k->n <= 0 || k->sample < 0) return 0;
    return launch_items(k_ss_rays, *k, k->n, stream);
}

extern "C" int bhrt_launch_ss_resolve(const bhrt_ss_resolve_k* k, void* stream) {
    if (k->n <= 0 || k->samples <= 0) return 0;
    return launch_items(k_ss_resolve, *k, k->n, stream);
}

extern "C" int bhrt_launch_ad_rays(const bhrt_ad_rays_k* k, void* stream) {
    if (k->n <= 0 || k->first < 0) return 0;
    return launch_items(k_ad_rays, *k, k->n, stream);
}

extern "C" int bhrt_launch_ad_edges(const bhrt_ad_edges_k* k, void* stream) {
    if (k->n <= 0 || k->base <= 0) return 0;
    return launch_items(k_ad_edges, *k, k->n, stream);
}

extern "C" int bhrt_launch_ad_resolve(const bhrt_ad_resolve_k* k, void* stream) {
    if (k->n <= 0 || k->base <= 0) return 0;
    return launch_items(k_ad_resolve, *k, k->n, stream);
}

extern "C" int bhrt_launch_ta_blend(const bhrt_ta_blend_k* k, void* stream) {
    if (k->n <= 0 || (k->stride != 3 && k->stride != 4)) return 0;
    return launch_items(k_ta_blend, *k, k->n, stream);
}

extern "C" int bhrt_launch_ta_edges(const bhrt_ta_edges_k* k, void* stream) {
    if (k->n <= 0 || k->width <= 0 || k->n != (long)k->width * k->height) return 0;
    return launch_items(k_ta_edges, *k, k->n, stream);
}
