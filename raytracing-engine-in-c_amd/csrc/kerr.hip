// kerr.hip -- physical null geodesics of Kerr in Cartesian Kerr-Schild coordinates: the kernel
// k_kerr and its launcher (the rule: include/bhrt_api.h "Physical geodesics"; tests/kerr_rule.py
// restates it in numpy; the host side is kerr.c), and k_kerr_paths, the same rays' recorded
// polylines (below k_kerr; the host side is kerr_paths.c), and k_kerr_rk45, the same rays by adaptive
// Dormand-Prince 5(4) attempts (below k_kerr_paths; the rule: "Physical geodesics, adaptive steps";
// the host side is kerr_rk45.c), and k_kerr_emit, the adaptive rays with recorded disk crossings,
// their redshift and intensity (below k_kerr_rk45; the rule: "Kerr disk emission"; the host side is
// kerr_emit.c).
//
// One lane per ray, FP64, fixed-step RK4 on (x, p), no LDS. A wavefront claims 64 rays at a time
// from the launch's claim counter -- an 8x8 pixel tile of a camera frame, so that its rays live
// alike, or 64 consecutive rays of an array -- and runs them until the last has ended; there is no
// refill of single lanes. Each stage forms the reciprocals of D, r, G and S once; the geometry at
// a step's end point serves the horizon test, the next step's size and the next step's first
// stage, so a step costs four geometry evaluations.
//
// ONE instantiation serves camera frames and ray arrays, with and without a disk, a sky map or
// the diagnostics (wave-uniform branches outside the stages): a ray's arithmetic is compiled once,
// so its outputs are the same bits through every entry point. No atomic touches an output; the
// claim counter and the statistics are the only atomics.
#include <hip/hip_runtime.h>

#include "bhrt_kernel.h"
#include "bhrt_launch.h"
#include "kerr_emit.h"
#include "kerr_init.h"

namespace {

using Scene = bhrt_scene_k;

#include "bhrt_colour.h"

constexpr double kDblMax = 1.79769313486231570815e+308;

struct Geom {
    double r, ir, iD, iG, iS, S, f, lx, ly, lz;
};

// the geometry at (x, y, z): two square roots, four reciprocals
__device__ __forceinline__ Geom geom(double x, double y, double z, const bhrt_kerr_k& k) {
    Geom g;
    const double z2 = z * z;
    const double rho2 = (x * x + y * y) + z2;
    const double w = rho2 - k.a2;
    const double az2 = k.a2 * z2;
    const double D = sqrt(w * w + 4.0 * az2);
    const double r2 = 0.5 * (w + D);
    g.r = sqrt(r2);
    const double G = r2 * r2 + az2;
    g.S = r2 + k.a2;
    g.ir = 1.0 / g.r;
    g.iD = 1.0 / D;
    g.iG = 1.0 / G;
    g.iS = 1.0 / g.S;
    g.f = k.two_m * (g.r * r2) * g.iG;
    g.lx = (g.r * x + k.a * y) * g.iS;
    g.ly = (g.r * y - k.a * x) * g.iS;
    g.lz = z * g.ir;
    return g;
}

// xdot_i = p_i - f u l_i, pdot_i = 1/2 (d_i f) u^2 + f u (d_i l_j) p_j with the analytic gradients;
// the terms of d_i l_j p_j that carry d_i r are gathered into one factor (Ap)
__device__ __forceinline__ void deriv(const Geom& g, double x, double y, double z, double px,
                                      double py, double pz, double E, const bhrt_kerr_k& k,
                                      double (&d)[6]) {
    const double u = E + ((g.lx * px + g.ly * py) + g.lz * pz);
    const double fu = g.f * u;
    d[0] = px - fu * g.lx;
    d[1] = py - fu * g.ly;
    d[2] = pz - fu * g.lz;
    const double rD = g.r * g.iD;
    const double drx = x * rD, dry = y * rD, drz = z * g.S * (g.ir * g.iD);
    const double r3 = g.r * g.r * g.r;
    const double q = g.f * (3.0 * g.ir - 4.0 * r3 * g.iG);
    const double hu2 = 0.5 * (u * u);
    const double t = 2.0 * g.r * g.iS;
    const double A = x * g.iS - g.lx * t, B = y * g.iS - g.ly * t, Cz = -z * (g.ir * g.ir);
    const double Ap = (A * px + B * py) + Cz * pz;
    d[3] = hu2 * (q * drx) + fu * (drx * Ap + (g.r * px - k.a * py) * g.iS);
    d[4] = hu2 * (q * dry) + fu * (dry * Ap + (k.a * px + g.r * py) * g.iS);
    d[5] = hu2 * (q * drz - g.f * (2.0 * k.a2 * z) * g.iG) + fu * (drz * Ap + g.ir * pz);
}

__device__ __forceinline__ bool finite6(const double (&y)[6]) {
    return fabs(y[0]) <= kDblMax && fabs(y[1]) <= kDblMax && fabs(y[2]) <= kDblMax &&
           fabs(y[3]) <= kDblMax && fabs(y[4]) <= kDblMax && fabs(y[5]) <= kDblMax;
}

// |(-E^2 + p.p - f u^2) / (E^2 + p.p + f u^2)| at a point whose geometry is g
__device__ __forceinline__ double h_residual(const Geom& g, const double (&y)[6], double E) {
    const double u = E + ((g.lx * y[3] + g.ly * y[4]) + g.lz * y[5]);
    const double pp = (y[3] * y[3] + y[4] * y[4]) + y[5] * y[5];
    const double fu2 = g.f * (u * u);
    return fabs(((pp - E * E) - fu2) / ((E * E + pp) + fu2));
}

// the direction of shard pixel (px, row j of the shard): calculate_ray_direction's mapping, one
// operation per rounding (tests/kerr_rule.py camera_dirs forms the same bits)
__device__ __forceinline__ void camera_dir(const bhrt_camera_k& cm, int px, int j, double (&d)[3]) {
#pragma clang fp contract(off)
    int py = j;
    if (cm.rows.num_shards > 1) {
        const int B = cm.rows.row_block, jb = j / B;
        py = (jb * cm.rows.num_shards + cm.rows.shard) * B + (j - jb * B);
    }
    const double ndcx = (2.0 * (((double)px + cm.off_x) / (double)cm.width) - 1.0) * cm.plane_w;
    const double ndcy = (1.0 - 2.0 * (((double)py + cm.off_y) / (double)cm.height)) * cm.plane_h;
    const double v[3] = {(cm.fwd[0] + cm.right[0] * ndcx) + cm.up[0] * ndcy,
                         (cm.fwd[1] + cm.right[1] * ndcx) + cm.up[1] * ndcy,
                         (cm.fwd[2] + cm.right[2] * ndcx) + cm.up[2] * ndcy};
    bhrt_kerr_unit(v, d);
}

// The launch parameters as an opaque pointer into the kernel argument segment (k_kerr's first
// argument starts it): the fields read through it -- the camera at a ray's set-up, the output
// pointers, the colour's constants and the sky map at its exit -- are loaded where they are used
// instead of being held in scalar registers across the steps.
typedef const __attribute__((address_space(4))) bhrt_kparams kparams_as4;
__device__ __forceinline__ const bhrt_kparams& in_kernarg(const bhrt_kparams&) {
    kparams_as4* p = (kparams_as4*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const bhrt_kparams*)p;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

__global__ __launch_bounds__(64) void k_kerr(const bhrt_kparams kp, const bhrt_kerr_k kk) {
    const int lane = threadIdx.x;
    const bhrt_kparams& kc = in_kernarg(kp);
    const bool camera = kp.src == BHRT_SRC_CAMERA;
    const bool diag = kk.h_residual != nullptr || kk.lz_drift != nullptr;
    const unsigned long long units =
        camera ? (unsigned long long)kk.ntiles : ((unsigned long long)kp.n + 63ull) / 64ull;
    if (lane == 0) atomicMax(kp.ctl + 8, ~(unsigned long long)wall_clock64());
    unsigned n_rays = 0, n_steps = 0;
    for (;;) {
        unsigned long long unit = 0;
        if (lane == 0) unit = atomicAdd(kp.ctl, 1ull);
        unit = __shfl(unit, 0);
        if (unit >= units) break;
        // the lane's ray: id i (the output element), origin and direction
        int i;
        bool live;
        double o[3], dir[3];
        if (camera) {
            const int ty = (int)unit / kk.tiles_x, tx = (int)unit - ty * kk.tiles_x;
            const int px = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
            live = px < kc.cam.width && j < kk.nrows;
            i = j * kc.cam.width + px;
            o[0] = kc.cam.pos[0];
            o[1] = kc.cam.pos[1];
            o[2] = kc.cam.pos[2];
            camera_dir(kc.cam, live ? px : 0, live ? j : 0, dir);
        } else {
            i = (int)unit * 64 + lane;
            live = i < kp.n;
            const Ray ray = kc.rays[live ? i : 0];
            o[0] = ray.origin.x;
            o[1] = ray.origin.y;
            o[2] = ray.origin.z;
            dir[0] = ray.direction.x;
            dir[1] = ray.direction.y;
            dir[2] = ray.direction.z;
        }
        double nv[3], l0[3], p0[3], f0, E;
        bhrt_kerr_unit(dir, nv);
        const bool observer =
            bhrt_kerr_origin(o[0], o[1], o[2], kk.a, kk.a2, kk.two_m, kk.r_plus, &f0, l0) != 0;
        bhrt_kerr_photon(f0, l0, nv, p0, &E);
        double y[6] = {o[0], o[1], o[2], p0[0], p0[1], p0[2]};
        int res = observer ? (kk.max_steps > 0 ? -1 : (int)RAY_MAX_STEPS) : (int)RAY_ERROR;
        int steps = 0;
        double dist = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
        Geom g = geom(y[0], y[1], y[2], kk);
        const double lz0 = y[0] * y[4] - y[1] * y[3];
        double hres = 0.0, lzd = 0.0;
        if (diag && observer) hres = h_residual(g, y, E);
        bool run = live && res < 0;
        while (__ballot(run) != 0ull) {
            if (run) {
                const double h = kk.dt * fmin(1.0, fmax(g.r / kk.eight_m, 0.0625));
                const double hh = 0.5 * h;
                double k1[6], k2[6], k3[6], k4[6], s[6];
                deriv(g, y[0], y[1], y[2], y[3], y[4], y[5], E, kk, k1);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + hh * k1[c];
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k2);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + hh * k2[c];
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k3);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + h * k3[c];
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k4);
                const double h6 = h / 6.0;
                double yn[6];
#pragma unroll
                for (int c = 0; c < 6; c++)
                    yn[c] = y[c] + h6 * ((k1[c] + 2.0 * k2[c]) + (2.0 * k3[c] + k4[c]));
                steps++;
                cx = yn[0] - y[0];
                cy = yn[1] - y[1];
                cz = yn[2] - y[2];
                const double seg = sqrt((cx * cx + cy * cy) + cz * cz);
                const Geom gn = geom(yn[0], yn[1], yn[2], kk);
                const double zo = y[2], zn = yn[2];
                if (!finite6(yn)) {  // 1. a non-finite state
                    res = RAY_ERROR;
                } else {
                    if (diag) {  // (the accepted point: before a disk hit replaces it)
                        hres = fmax(hres, h_residual(gn, yn, E));
                        lzd = fabs((yn[0] * yn[4] - yn[1] * yn[3]) - lz0);
                    }
                    if (kk.has_disk && ((zo > 0.0 && zn <= 0.0) || (zo < 0.0 && zn >= 0.0))) {
                        const double t = zo / (zo - zn);  // 2. the disk
                        const double qx = y[0] + t * cx, qy = y[1] + t * cy;
                        const double s2 = qx * qx + qy * qy;
                        if (kk.disk_lo <= s2 && s2 <= kk.disk_hi) {
                            res = RAY_DISK;
                            yn[0] = qx;
                            yn[1] = qy;
                            yn[2] = 0.0;
                            dist += t * seg;
                        }
                    }
                    if (res < 0) {
                        if (gn.r <= kk.r_plus) {  // 3. the horizon
                            res = RAY_HORIZON;
                        } else {
                            dist += seg;  // 4. the distance
                            if (dist > kk.max_dist) res = RAY_MAX_DISTANCE;
                            else if (steps >= kk.max_steps) res = RAY_MAX_STEPS;  // 5.
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < 6; c++) y[c] = yn[c];
                g = gn;
                run = res < 0;
            }
        }
        if (!live) continue;
        n_rays++;
        n_steps += (unsigned)steps;
        const bhrt_frame_soa& out = kc.out;
        if (out.result) out.result[i] = res;
        if (out.steps) out.steps[i] = steps;
        if (out.hit_x) out.hit_x[i] = y[0];
        if (out.hit_y) out.hit_y[i] = y[1];
        if (out.hit_z) out.hit_z[i] = y[2];
        if (out.distance) out.distance[i] = dist;
        if (res == RAY_MAX_DISTANCE) {
            if (out.sky_x) out.sky_x[i] = cx;
            if (out.sky_y) out.sky_y[i] = cy;
            if (out.sky_z) out.sky_z[i] = cz;
        }
        if (kk.h_residual) kk.h_residual[i] = hres;
        if (kk.lz_drift) kk.lz_drift[i] = lzd;
        if (out.rgb_r || out.rgba32f || out.rgba8) {
            // the unit chord of the last segment: the Doppler direction of a disk hit, and what
            // the gradient reads for a ray that left the scene; every other ray reads n
            double uc[3];
            const double c3[3] = {cx, cy, cz};
            bhrt_kerr_unit(c3, uc);
            double r, gg, b;
            if ((kc.sc.flags & BHRT_FLAG_SKY) && res != RAY_DISK && res != RAY_HORIZON) {
                // the sky-map rule: the exit chord of a ray that left the scene if it counts
                // (finite, squared length > 0), else n. Inlined here, not colour_of_sky's call:
                // that function returns through memory, and this kernel has one instantiation,
                // so there is no second copy of the iterations to keep in step with
                const double l2 = (cx * cx + cy * cy) + cz * cz;
                const bool take = res == RAY_MAX_DISTANCE && fabs(cx) <= kDblMax &&
                                  fabs(cy) <= kDblMax && fabs(cz) <= kDblMax && l2 > 0.0;
                sky_lookup(kc.sky, take ? cx : nv[0], take ? cy : nv[1], take ? cz : nv[2], r, gg,
                           b);
            } else {
                const bool chord = res == RAY_DISK || res == RAY_MAX_DISTANCE;
                colour_of(kc.sc, res, y[0], y[1], chord ? uc[0] : nv[0], chord ? uc[1] : nv[1],
                          chord ? uc[2] : nv[2], r, gg, b);
            }
            store_colour(out, i, r, gg, b);
        }
    }
    const unsigned long long s0 = wave_sum(n_rays), s1 = wave_sum(n_steps);
    if (lane == 0) {
        atomicMax(kp.ctl + 9, (unsigned long long)wall_clock64());
        if (s0) atomicAdd(kp.ctl + 1, s0);
        if (s1) atomicAdd(kp.ctl + 2, s1);
    }
}

// The recorded polylines of a ray array (the rule: include/bhrt_api.h "Physical photon paths";
// tests/kerr_paths_rule.py restates it; the host side is kerr_paths.c). k_kerr's ray-array branch
// and k_kerr's step -- geom, deriv, finite6, the five tests in the rule's order, kerr_init.h's
// initial data -- without colour, sky map or diagnostics, and with the point stores. The loop is
// written out a second time, not shared through an inline function: with the step factored out of
// k_kerr the compiler allocated k_kerr's registers differently, and k_kerr's
// device code is to stay what it was.
// Point j of the full path is the position after step j (steps == j; q_0 the origin), the hit
// point for the step that hits the disk. A lane keeps the multiples of `every` (next_keep: the next
// one) and, at its end, the last point if that was not one; `slot` counts what it stored, and
// nothing is stored from max_positions on. Steps advance one at a time, so one test per step
// decides. Direct stores: the lane writes its 24 B point (12 B of xyz32) where it is produced.
__global__ __launch_bounds__(64) void k_kerr_paths(const bhrt_kparams kp,
                                                   const bhrt_kerr_paths_k pk) {
    const int lane = threadIdx.x;
    const bhrt_kerr_k& kk = pk.k;
    const size_t P = (size_t)pk.max_positions;
    const long long every = pk.every;
    double* const xyz = reinterpret_cast<double*>(pk.out.xyz);
    float* const xyz32 = pk.out.xyz32;
    const unsigned long long units = ((unsigned long long)kp.n + 63ull) / 64ull;
    if (lane == 0) atomicMax(kp.ctl + 8, ~(unsigned long long)wall_clock64());
    unsigned n_rays = 0, n_steps = 0;
    for (;;) {
        unsigned long long unit = 0;
        if (lane == 0) unit = atomicAdd(kp.ctl, 1ull);
        unit = __shfl(unit, 0);
        if (unit >= units) break;
        const unsigned long long id = unit * 64ull + (unsigned)lane;
        const bool live = id < (unsigned long long)kp.n;
        const int i = live ? (int)id : 0;
        const size_t row = (size_t)i * P;  // element index of the ray's slot 0
        const Ray ray = kp.rays[i];
        const double o[3] = {ray.origin.x, ray.origin.y, ray.origin.z};
        const double dir[3] = {ray.direction.x, ray.direction.y, ray.direction.z};
        double nv[3], l0[3], p0[3], f0, E;
        bhrt_kerr_unit(dir, nv);
        const bool observer =
            bhrt_kerr_origin(o[0], o[1], o[2], kk.a, kk.a2, kk.two_m, kk.r_plus, &f0, l0) != 0;
        bhrt_kerr_photon(f0, l0, nv, p0, &E);
        double y[6] = {o[0], o[1], o[2], p0[0], p0[1], p0[2]};
        int res = observer ? (kk.max_steps > 0 ? -1 : (int)RAY_MAX_STEPS) : (int)RAY_ERROR;
        int steps = 0;
        double dist = 0.0;
        Geom g = geom(y[0], y[1], y[2], kk);
        size_t slot = 0;          // points stored (or counted, without a point output)
        long long next_keep = 0;  // the next path index that is kept
        // the point y[0..2] is kept: into slot `slot` (the caller checked live and slot < P)
        auto emit = [&]() {
            const size_t e = (row + slot) * 3;
            if (xyz) {
                xyz[e] = y[0];
                xyz[e + 1] = y[1];
                xyz[e + 2] = y[2];
            }
            if (xyz32) {
                xyz32[e] = (float)y[0];
                xyz32[e + 1] = (float)y[1];
                xyz32[e + 2] = (float)y[2];
            }
            slot++;
            next_keep += every;
        };
        if (live) emit();  // q_0, the origin as given; max_positions >= 1
        bool run = live && res < 0;
        while (__ballot(run) != 0ull) {
            if (run) {
                const double h = kk.dt * fmin(1.0, fmax(g.r / kk.eight_m, 0.0625));
                const double hh = 0.5 * h;
                double k1[6], k2[6], k3[6], k4[6], s[6];
                deriv(g, y[0], y[1], y[2], y[3], y[4], y[5], E, kk, k1);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + hh * k1[c];
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k2);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + hh * k2[c];
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k3);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + h * k3[c];
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k4);
                const double h6 = h / 6.0;
                double yn[6];
#pragma unroll
                for (int c = 0; c < 6; c++)
                    yn[c] = y[c] + h6 * ((k1[c] + 2.0 * k2[c]) + (2.0 * k3[c] + k4[c]));
                steps++;
                const double cx = yn[0] - y[0], cy = yn[1] - y[1], cz = yn[2] - y[2];
                const double seg = sqrt((cx * cx + cy * cy) + cz * cz);
                const Geom gn = geom(yn[0], yn[1], yn[2], kk);
                const double zo = y[2], zn = yn[2];
                if (!finite6(yn)) {  // 1. a non-finite state
                    res = RAY_ERROR;
                } else {
                    if (kk.has_disk && ((zo > 0.0 && zn <= 0.0) || (zo < 0.0 && zn >= 0.0))) {
                        const double t = zo / (zo - zn);  // 2. the disk
                        const double qx = y[0] + t * cx, qy = y[1] + t * cy;
                        const double s2 = qx * qx + qy * qy;
                        if (kk.disk_lo <= s2 && s2 <= kk.disk_hi) {
                            res = RAY_DISK;
                            yn[0] = qx;
                            yn[1] = qy;
                            yn[2] = 0.0;
                            dist += t * seg;
                        }
                    }
                    if (res < 0) {
                        if (gn.r <= kk.r_plus) {  // 3. the horizon
                            res = RAY_HORIZON;
                        } else {
                            dist += seg;  // 4. the distance
                            if (dist > kk.max_dist) res = RAY_MAX_DISTANCE;
                            else if (steps >= kk.max_steps) res = RAY_MAX_STEPS;  // 5.
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < 6; c++) y[c] = yn[c];
                g = gn;
                run = res < 0;
                // q_steps: a kept index, or the end of the ray unless it was just kept (next_keep -
                // every: the last kept index; a truncated ray stores no more)
                if (slot < P && (next_keep == (long long)steps ||
                                 (!run && next_keep - every != (long long)steps)))
                    emit();
            }
        }
        if (!live) continue;
        n_rays++;
        n_steps += (unsigned)steps;
        if (pk.out.count) pk.out.count[i] = (int)slot;
    }
    const unsigned long long s0 = wave_sum(n_rays), s1 = wave_sum(n_steps);
    if (lane == 0) {
        atomicMax(kp.ctl + 9, (unsigned long long)wall_clock64());
        if (s0) atomicAdd(kp.ctl + 1, s0);
        if (s1) atomicAdd(kp.ctl + 2, s1);
    }
}

// The adaptive rays (the rule: include/bhrt_api.h "Physical geodesics, adaptive steps";
// tests/kerr_rk45_rule.py restates it; the host side is kerr_rk45.c). k_kerr's shape -- the claim
// of tiles or 64 rays, the set-up, the outputs, the colour, the statistics -- around Dormand-Prince
// 5(4) attempts on the shared geom / deriv / finite6. FSAL: k1 and g are the accepted point's
// stage 7 and geometry, kept across attempts (a rejected attempt keeps them), so an attempt costs
// six geometry and derivative evaluations. The loop is a third copy for k_kerr_paths' reason:
// k_kerr's device code is to stay what it was. Lanes of a wave take different numbers of attempts
// and wait for the longest; there is no refill of single lanes.
// Occupancy: two waves per SIMD, 256 registers per lane, no scratch. To fit them, what is live
// across the stages is kept small: the sums of ynew and e over stages 1..5 are formed with stage
// 6's point, n is formed again at the ray's exit, and the exit tangent is read from k1
// (profiles/kerr_rk45/resource_usage.txt).
constexpr int kRk45Waves = 2;

// the standard Dormand-Prince tableau; kE = b5 - b4
constexpr double kA21 = 1.0 / 5.0;
constexpr double kA31 = 3.0 / 40.0, kA32 = 9.0 / 40.0;
constexpr double kA41 = 44.0 / 45.0, kA42 = -56.0 / 15.0, kA43 = 32.0 / 9.0;
constexpr double kA51 = 19372.0 / 6561.0, kA52 = -25360.0 / 2187.0, kA53 = 64448.0 / 6561.0,
                 kA54 = -212.0 / 729.0;
constexpr double kA61 = 9017.0 / 3168.0, kA62 = -355.0 / 33.0, kA63 = 46732.0 / 5247.0,
                 kA64 = 49.0 / 176.0, kA65 = -5103.0 / 18656.0;
constexpr double kB1 = 35.0 / 384.0, kB3 = 500.0 / 1113.0, kB4 = 125.0 / 192.0,
                 kB5 = -2187.0 / 6784.0, kB6 = 11.0 / 84.0;
constexpr double kE1 = 71.0 / 57600.0, kE3 = -71.0 / 16695.0, kE4 = 71.0 / 1920.0,
                 kE5 = -17253.0 / 339200.0, kE6 = 22.0 / 525.0, kE7 = -1.0 / 40.0;

__global__ __launch_bounds__(64, kRk45Waves) void k_kerr_rk45(const bhrt_kparams kp,
                                                              const bhrt_kerr_rk45_k rk) {
    const int lane = threadIdx.x;
    const bhrt_kparams& kc = in_kernarg(kp);
    const bhrt_kerr_k& kk = rk.k;
    const bool camera = kp.src == BHRT_SRC_CAMERA;
    const bool diag = kk.h_residual != nullptr || kk.lz_drift != nullptr;
    const unsigned long long units =
        camera ? (unsigned long long)kk.ntiles : ((unsigned long long)kp.n + 63ull) / 64ull;
    if (lane == 0) atomicMax(kp.ctl + 8, ~(unsigned long long)wall_clock64());
    unsigned n_rays = 0, n_steps = 0;
    for (;;) {
        unsigned long long unit = 0;
        if (lane == 0) unit = atomicAdd(kp.ctl, 1ull);
        unit = __shfl(unit, 0);
        if (unit >= units) break;
        // the lane's ray: id i (the output element), origin and direction (as k_kerr)
        int i;
        bool live;
        double o[3], dir[3];
        if (camera) {
            const int ty = (int)unit / kk.tiles_x, tx = (int)unit - ty * kk.tiles_x;
            const int px = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
            live = px < kc.cam.width && j < kk.nrows;
            i = j * kc.cam.width + px;
            o[0] = kc.cam.pos[0];
            o[1] = kc.cam.pos[1];
            o[2] = kc.cam.pos[2];
            camera_dir(kc.cam, live ? px : 0, live ? j : 0, dir);
        } else {
            i = (int)unit * 64 + lane;
            live = i < kp.n;
            const Ray ray = kc.rays[live ? i : 0];
            o[0] = ray.origin.x;
            o[1] = ray.origin.y;
            o[2] = ray.origin.z;
            dir[0] = ray.direction.x;
            dir[1] = ray.direction.y;
            dir[2] = ray.direction.z;
        }
        double l0[3], p0[3], f0, E;
        const bool observer =
            bhrt_kerr_origin(o[0], o[1], o[2], kk.a, kk.a2, kk.two_m, kk.r_plus, &f0, l0) != 0;
        {
            double nv[3];
            bhrt_kerr_unit(dir, nv);
            bhrt_kerr_photon(f0, l0, nv, p0, &E);
        }
        double y[6] = {o[0], o[1], o[2], p0[0], p0[1], p0[2]};
        int res = observer ? (kk.max_steps > 0 ? -1 : (int)RAY_MAX_STEPS) : (int)RAY_ERROR;
        int steps = 0, rejected = 0;  // attempts, and those not accepted
        double dist = 0.0;
        Geom g = geom(y[0], y[1], y[2], kk);
        const double lz0 = y[0] * y[4] - y[1] * y[3];
        double hres = 0.0, lzd = 0.0;
        if (diag && observer) hres = h_residual(g, y, E);
        double k1[6];
        deriv(g, y[0], y[1], y[2], y[3], y[4], y[5], E, kk, k1);
        double hnext = kk.dt;
        bool run = live && res < 0;
        while (__ballot(run) != 0ull) {
            if (run) {
                const double h = fmin(hnext, 0.5 * g.r);  // no attempt leaps the hole
                double k2[6], k3[6], k4[6], k5[6], k6[6], k7[6], s[6], yn[6];
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + h * (kA21 * k1[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k2);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + h * (kA31 * k1[c] + kA32 * k2[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k3);
#pragma unroll
                for (int c = 0; c < 6; c++)
                    s[c] = y[c] + h * ((kA41 * k1[c] + kA42 * k2[c]) + kA43 * k3[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k4);
#pragma unroll
                for (int c = 0; c < 6; c++)
                    s[c] = y[c] +
                           h * (((kA51 * k1[c] + kA52 * k2[c]) + kA53 * k3[c]) + kA54 * k4[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k5);
                // the sums of ynew and e over stages 1..5 are formed here, in the rule's order, so
                // that k2..k5 end with stage 6's point
                double bs[6], es[6];
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    s[c] = y[c] + h * ((((kA61 * k1[c] + kA62 * k2[c]) + kA63 * k3[c]) +
                                        kA64 * k4[c]) + kA65 * k5[c]);
                    bs[c] = ((kB1 * k1[c] + kB3 * k3[c]) + kB4 * k4[c]) + kB5 * k5[c];
                    es[c] = ((kE1 * k1[c] + kE3 * k3[c]) + kE4 * k4[c]) + kE5 * k5[c];
                }
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k6);
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    yn[c] = y[c] + h * (bs[c] + kB6 * k6[c]);
                    es[c] = es[c] + kE6 * k6[c];
                }
                const Geom gn = geom(yn[0], yn[1], yn[2], kk);
                deriv(gn, yn[0], yn[1], yn[2], yn[3], yn[4], yn[5], E, kk, k7);
                // err = max_c |e_c| / (tol (1 + max(|y_c|, |ynew_c|))), e = h sum (b5 - b4)_j k_j
                double err = 0.0;
                bool err_nan = false;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const double e = h * (es[c] + kE7 * k7[c]);
                    const double q = fabs(e) / (rk.tol * (1.0 + fmax(fabs(y[c]), fabs(yn[c]))));
                    err_nan = err_nan || q != q;
                    err = fmax(err, q);
                }
                steps++;
                if (!finite6(yn) || err_nan || !(err <= kDblMax)) {  // 1. a non-finite attempt
                    res = RAY_ERROR;
#pragma unroll
                    for (int c = 0; c < 6; c++) y[c] = yn[c];
                } else {
                    double fac = fmin(5.0, fmax(0.2, 0.9 * pow(err, -0.2)));
                    if (!(fabs(fac) <= kDblMax)) fac = 0.2;
                    hnext = h * fac;
                    if (err <= 1.0) {  // accepted; a rejected attempt goes to test 6 alone
                        if (diag) {    // (the accepted point: before a disk hit replaces it)
                            hres = fmax(hres, h_residual(gn, yn, E));
                            lzd = fabs((yn[0] * yn[4] - yn[1] * yn[3]) - lz0);
                        }
                        const double cx = yn[0] - y[0], cy = yn[1] - y[1], cz = yn[2] - y[2];
                        const double seg = sqrt((cx * cx + cy * cy) + cz * cz);
                        const double zo = y[2], zn = yn[2];
                        if (kk.has_disk && ((zo > 0.0 && zn <= 0.0) || (zo < 0.0 && zn >= 0.0))) {
                            // 3. the disk, on the step's cubic Hermite polynomials
                            // q(th) = q_old + th (m0 + th (c2 + th c3))
                            const double d3[3] = {cx, cy, cz};
                            double m0[3], c2[3], c3[3];
#pragma unroll
                            for (int c = 0; c < 3; c++) {
                                m0[c] = h * k1[c];
                                const double m1 = h * k7[c];
                                c2[c] = (3.0 * d3[c] - 2.0 * m0[c]) - m1;
                                c3[c] = (m0[c] + m1) - 2.0 * d3[c];
                            }
                            double th = zo / (zo - zn);
#pragma unroll
                            for (int it = 0; it < 4; it++) {
                                const double pz = zo + th * (m0[2] + th * (c2[2] + th * c3[2]));
                                const double dz = m0[2] + th * (2.0 * c2[2] + th * (3.0 * c3[2]));
                                const double tn = th - pz / dz;
                                if (fabs(tn) <= kDblMax) th = fmin(1.0, fmax(0.0, tn));
                            }
                            const double qx = y[0] + th * (m0[0] + th * (c2[0] + th * c3[0]));
                            const double qy = y[1] + th * (m0[1] + th * (c2[1] + th * c3[1]));
                            const double s2 = qx * qx + qy * qy;
                            if (kk.disk_lo <= s2 && s2 <= kk.disk_hi) {
                                res = RAY_DISK;
                                yn[0] = qx;
                                yn[1] = qy;
                                yn[2] = 0.0;
                                dist += th * seg;
                                // (the ray ends here: k7, the next k1, carries the tangent out)
#pragma unroll
                                for (int c = 0; c < 3; c++)
                                    k7[c] = m0[c] + th * (2.0 * c2[c] + th * (3.0 * c3[c]));
                            }
                        }
                        if (res < 0) {
                            if (gn.r <= kk.r_plus) {  // 4. the horizon
                                res = RAY_HORIZON;
                            } else {
                                dist += seg;  // 5. the distance
                                if (dist > kk.max_dist) res = RAY_MAX_DISTANCE;
                            }
                        }
#pragma unroll
                        for (int c = 0; c < 6; c++) {
                            y[c] = yn[c];
                            k1[c] = k7[c];
                        }
                        g = gn;
                    } else {
                        rejected++;
                    }
                    if (res < 0 && steps >= kk.max_steps) res = RAY_MAX_STEPS;  // 6.
                }
                run = res < 0;
            }
        }
        if (!live) continue;
        // the tangent at the last point: k1 is an accepted attempt's stage 7 (xdot at its end) or
        // the Hermite derivative at a disk hit; read for RAY_DISK and RAY_MAX_DISTANCE rays only
        const double tx = k1[0], ty = k1[1], tz = k1[2];
        n_rays++;
        n_steps += (unsigned)steps;
        const bhrt_frame_soa& out = kc.out;
        if (out.result) out.result[i] = res;
        if (out.steps) out.steps[i] = steps;
        if (out.hit_x) out.hit_x[i] = y[0];
        if (out.hit_y) out.hit_y[i] = y[1];
        if (out.hit_z) out.hit_z[i] = y[2];
        if (out.distance) out.distance[i] = dist;
        if (res == RAY_MAX_DISTANCE) {
            if (out.sky_x) out.sky_x[i] = tx;
            if (out.sky_y) out.sky_y[i] = ty;
            if (out.sky_z) out.sky_z[i] = tz;
        }
        if (kk.h_residual) kk.h_residual[i] = hres;
        if (kk.lz_drift) kk.lz_drift[i] = lzd;
        if (rk.rejected) rk.rejected[i] = rejected;
        if (out.rgb_r || out.rgba32f || out.rgba8) {
            // the unit tangent at the last point: the Doppler direction of a disk hit, and what
            // the gradient reads for a ray that left the scene; every other ray reads n
            double ut[3];
            const double t3[3] = {tx, ty, tz};
            bhrt_kerr_unit(t3, ut);
            // n again, by the set-up's own operations: not held across the attempts
            double nv[3];
            if (camera) {
                camera_dir(kc.cam, i % kc.cam.width, i / kc.cam.width, dir);
            } else {
                const Ray ray = kc.rays[i];
                dir[0] = ray.direction.x;
                dir[1] = ray.direction.y;
                dir[2] = ray.direction.z;
            }
            bhrt_kerr_unit(dir, nv);
            double r, gg, b;
            if ((kc.sc.flags & BHRT_FLAG_SKY) && res != RAY_DISK && res != RAY_HORIZON) {
                // the sky-map rule on the exit tangent (k_kerr's lookup, inlined for its reason)
                const double l2 = (tx * tx + ty * ty) + tz * tz;
                const bool take = res == RAY_MAX_DISTANCE && fabs(tx) <= kDblMax &&
                                  fabs(ty) <= kDblMax && fabs(tz) <= kDblMax && l2 > 0.0;
                sky_lookup(kc.sky, take ? tx : nv[0], take ? ty : nv[1], take ? tz : nv[2], r, gg,
                           b);
            } else {
                const bool tang = res == RAY_DISK || res == RAY_MAX_DISTANCE;
                colour_of(kc.sc, res, y[0], y[1], tang ? ut[0] : nv[0], tang ? ut[1] : nv[1],
                          tang ? ut[2] : nv[2], r, gg, b);
            }
            store_colour(out, i, r, gg, b);
        }
    }
    const unsigned long long s0 = wave_sum(n_rays), s1 = wave_sum(n_steps);
    if (lane == 0) {
        atomicMax(kp.ctl + 9, (unsigned long long)wall_clock64());
        if (s0) atomicAdd(kp.ctl + 1, s0);
        if (s1) atomicAdd(kp.ctl + 2, s1);
    }
}

// Disk emission (the rule: include/bhrt_api.h "Kerr disk emission"; tests/kerr_emit_rule.py
// restates it; the host side is kerr_emit.c). k_kerr_rk45's attempts, tests and exit, with the
// disk test recording up to K crossings per ray instead of ending the ray on its first: each
// crossing's radius and redshift (kerr_emit.h) are stored where the crossing is found -- after the
// attempt's state update, outside the stages, and rare. k_kerr_rk45 uses every register of its
// two-wave bound, so nothing of the emission is held in registers across the stages: the count,
// the intensity sum and the three colour sums wait in LDS between crossings, and so does what a
// ray touches once per accepted attempt at the most (L_z of the initial data, the distance, the two
// diagnostics); 76 bytes per lane, each lane its own words: no barrier. The loop is a fourth copy
// for k_kerr_paths' reason: the other kernels' device code is to stay what it was. Two waves per
// SIMD, 256 registers, no scratch (profiles/kerr_emit/resource_usage.txt).
constexpr int kEmitWaves = 2;

__global__ __launch_bounds__(64, kEmitWaves) void k_kerr_emit(const bhrt_kparams kp,
                                                              const bhrt_kerr_emit_k ek) {
    // What a ray reads or writes once per accepted attempt at the most waits in LDS, each lane its
    // own words (no barrier): one object, so that a lane's one address serves every slot.
    __shared__ struct {
        double sum[4][64];   // the sums of w_k and of w_k base_k (r, g, b)
        double sq[64];       // q_x^2 + q_y^2 of the attempt's crossing
        double lz0[64];      // L_z of the initial data
        double diag[2][64];  // h_residual, lz_drift
        double dist[64];     // distance
        int cnt[64];         // crossings recorded
    } ls;
    const int lane = threadIdx.x;
    const bhrt_kparams& kc = in_kernarg(kp);
    // the emission's parameters and outputs, read where a crossing or an exit uses them: the
    // second argument's place in the kernel argument segment, through the same opaque pointer
    const bhrt_kerr_emit_k& ec = *reinterpret_cast<const bhrt_kerr_emit_k*>(
        reinterpret_cast<const char*>(&kc) + ((sizeof(bhrt_kparams) + 7) & ~(size_t)7));
    const bhrt_kerr_rk45_k& rk = ek.rk;
    const bhrt_kerr_k& kk = rk.k;
    const bool camera = kp.src == BHRT_SRC_CAMERA;
    const bool diag = kk.h_residual != nullptr || kk.lz_drift != nullptr;
    const unsigned long long units =
        camera ? (unsigned long long)kk.ntiles : ((unsigned long long)kp.n + 63ull) / 64ull;
    if (lane == 0) atomicMax(kp.ctl + 8, ~(unsigned long long)wall_clock64());
    unsigned n_rays = 0, n_steps = 0;
    for (;;) {
        unsigned long long unit = 0;
        if (lane == 0) unit = atomicAdd(kp.ctl, 1ull);
        unit = __shfl(unit, 0);
        if (unit >= units) break;
        // the lane's ray: id i (the output element), origin and direction (as k_kerr)
        int i;
        bool live;
        double o[3], dir[3];
        if (camera) {
            const int ty = (int)unit / kk.tiles_x, tx = (int)unit - ty * kk.tiles_x;
            const int px = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
            live = px < kc.cam.width && j < kk.nrows;
            i = j * kc.cam.width + px;
            o[0] = kc.cam.pos[0];
            o[1] = kc.cam.pos[1];
            o[2] = kc.cam.pos[2];
            camera_dir(kc.cam, live ? px : 0, live ? j : 0, dir);
        } else {
            i = (int)unit * 64 + lane;
            live = i < kp.n;
            const Ray ray = kc.rays[live ? i : 0];
            o[0] = ray.origin.x;
            o[1] = ray.origin.y;
            o[2] = ray.origin.z;
            dir[0] = ray.direction.x;
            dir[1] = ray.direction.y;
            dir[2] = ray.direction.z;
        }
        double l0[3], p0[3], f0, E;
        const bool observer =
            bhrt_kerr_origin(o[0], o[1], o[2], kk.a, kk.a2, kk.two_m, kk.r_plus, &f0, l0) != 0;
        {
            double nv[3];
            bhrt_kerr_unit(dir, nv);
            bhrt_kerr_photon(f0, l0, nv, p0, &E);
        }
        double y[6] = {o[0], o[1], o[2], p0[0], p0[1], p0[2]};
        int res = observer ? (kk.max_steps > 0 ? -1 : (int)RAY_MAX_STEPS) : (int)RAY_ERROR;
        int steps = 0, rejected = 0;  // attempts, and those not accepted
        ls.dist[lane] = 0.0;  // the distance: read and written once per accepted attempt
        Geom g = geom(y[0], y[1], y[2], kk);
        // L_z of the initial data: read at a crossing and by the diagnostics, so it waits in LDS
        ls.lz0[lane] = y[0] * y[4] - y[1] * y[3];
        // (the diagnostics' two values as well: updated once per accepted attempt)
        ls.diag[0][lane] = (diag && observer) ? h_residual(g, y, E) : 0.0;
        ls.diag[1][lane] = 0.0;
        double k1[6];
        deriv(g, y[0], y[1], y[2], y[3], y[4], y[5], E, kk, k1);
        double hnext = kk.dt;
        // the lane's crossings so far, and its sums of w_k and of w_k base_k (r, g, b): in LDS, read
        // and written by this lane alone, at a crossing and at the ray's exit
        ls.cnt[lane] = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) ls.sum[c][lane] = 0.0;
        bool run = live && res < 0;
        while (__ballot(run) != 0ull) {
            if (run) {
                const double h = fmin(hnext, 0.5 * g.r);  // no attempt leaps the hole
                double k2[6], k3[6], k4[6], k5[6], k6[6], k7[6], s[6], yn[6];
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + h * (kA21 * k1[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k2);
#pragma unroll
                for (int c = 0; c < 6; c++) s[c] = y[c] + h * (kA31 * k1[c] + kA32 * k2[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k3);
#pragma unroll
                for (int c = 0; c < 6; c++)
                    s[c] = y[c] + h * ((kA41 * k1[c] + kA42 * k2[c]) + kA43 * k3[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k4);
#pragma unroll
                for (int c = 0; c < 6; c++)
                    s[c] = y[c] +
                           h * (((kA51 * k1[c] + kA52 * k2[c]) + kA53 * k3[c]) + kA54 * k4[c]);
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k5);
                // (the sums over stages 1..5 with stage 6's point, as k_kerr_rk45)
                double bs[6], es[6];
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    s[c] = y[c] + h * ((((kA61 * k1[c] + kA62 * k2[c]) + kA63 * k3[c]) +
                                        kA64 * k4[c]) + kA65 * k5[c]);
                    bs[c] = ((kB1 * k1[c] + kB3 * k3[c]) + kB4 * k4[c]) + kB5 * k5[c];
                    es[c] = ((kE1 * k1[c] + kE3 * k3[c]) + kE4 * k4[c]) + kE5 * k5[c];
                }
                deriv(geom(s[0], s[1], s[2], kk), s[0], s[1], s[2], s[3], s[4], s[5], E, kk, k6);
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    yn[c] = y[c] + h * (bs[c] + kB6 * k6[c]);
                    es[c] = es[c] + kE6 * k6[c];
                }
                const Geom gn = geom(yn[0], yn[1], yn[2], kk);
                deriv(gn, yn[0], yn[1], yn[2], yn[3], yn[4], yn[5], E, kk, k7);
                double err = 0.0;
                bool err_nan = false;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const double e = h * (es[c] + kE7 * k7[c]);
                    const double q = fabs(e) / (rk.tol * (1.0 + fmax(fabs(y[c]), fabs(yn[c]))));
                    err_nan = err_nan || q != q;
                    err = fmax(err, q);
                }
                steps++;
                if (!finite6(yn) || err_nan || !(err <= kDblMax)) {  // 1. a non-finite attempt
                    res = RAY_ERROR;
#pragma unroll
                    for (int c = 0; c < 6; c++) y[c] = yn[c];
                } else {
                    double fac = fmin(5.0, fmax(0.2, 0.9 * pow(err, -0.2)));
                    if (!(fabs(fac) <= kDblMax)) fac = 0.2;
                    hnext = h * fac;
                    if (err <= 1.0) {  // accepted; a rejected attempt goes to test 6 alone
                        if (diag) {    // (the accepted point: before a disk hit replaces it)
                            ls.diag[0][lane] = fmax(ls.diag[0][lane], h_residual(gn, yn, E));
                            ls.diag[1][lane] = fabs((yn[0] * yn[4] - yn[1] * yn[3]) - ls.lz0[lane]);
                        }
                        const double cx = yn[0] - y[0], cy = yn[1] - y[1], cz = yn[2] - y[2];
                        const double seg = sqrt((cx * cx + cy * cy) + cz * cz);
                        const double zo = y[2], zn = yn[2];
                        bool crossed = false;  // (q_x^2 + q_y^2 of the crossing waits in LDS)
                        if (kk.has_disk && ((zo > 0.0 && zn <= 0.0) || (zo < 0.0 && zn >= 0.0))) {
                            // 3. the disk, on the step's cubic Hermite polynomials (k_kerr_rk45's)
                            const double d3[3] = {cx, cy, cz};
                            double m0[3], c2[3], c3[3];
#pragma unroll
                            for (int c = 0; c < 3; c++) {
                                m0[c] = h * k1[c];
                                const double m1 = h * k7[c];
                                c2[c] = (3.0 * d3[c] - 2.0 * m0[c]) - m1;
                                c3[c] = (m0[c] + m1) - 2.0 * d3[c];
                            }
                            double th = zo / (zo - zn);
#pragma unroll
                            for (int it = 0; it < 4; it++) {
                                const double pz = zo + th * (m0[2] + th * (c2[2] + th * c3[2]));
                                const double dz = m0[2] + th * (2.0 * c2[2] + th * (3.0 * c3[2]));
                                const double tn = th - pz / dz;
                                if (fabs(tn) <= kDblMax) th = fmin(1.0, fmax(0.0, tn));
                            }
                            const double qx = y[0] + th * (m0[0] + th * (c2[0] + th * c3[0]));
                            const double qy = y[1] + th * (m0[1] + th * (c2[1] + th * c3[1]));
                            const double s2 = qx * qx + qy * qy;
                            if (kk.disk_lo <= s2 && s2 <= kk.disk_hi) {
                                // crossing number cnt (the K-th ends the ray); it is recorded
                                // below, once the attempt's stage vectors are dead
                                crossed = true;
                                ls.sq[lane] = s2;
                                if (ls.cnt[lane] + 1 == ec.max_crossings) {
                                    res = RAY_DISK;
                                    yn[0] = qx;
                                    yn[1] = qy;
                                    yn[2] = 0.0;
                                    ls.dist[lane] = ls.dist[lane] + th * seg;
                                    // (the ray ends here: k7, the next k1, carries the tangent out)
#pragma unroll
                                    for (int c = 0; c < 3; c++)
                                        k7[c] = m0[c] + th * (2.0 * c2[c] + th * (3.0 * c3[c]));
                                }
                            }
                        }
                        if (res < 0) {
                            if (gn.r <= kk.r_plus) {  // 4. the horizon
                                res = RAY_HORIZON;
                            } else {
                                const double dist = ls.dist[lane] + seg;  // 5. the distance
                                ls.dist[lane] = dist;
                                if (dist > kk.max_dist) res = RAY_MAX_DISTANCE;
                            }
                        }
#pragma unroll
                        for (int c = 0; c < 6; c++) {
                            y[c] = yn[c];
                            k1[c] = k7[c];
                        }
                        g = gn;
                        if (crossed) {
                            // the crossing's radius and redshift go to memory here, its weight
                            // into the sums
#pragma clang fp contract(off)
                            const double sq = ls.sq[lane];
                            const double rad = sqrt(sq - kk.a2);
                            const double gz = bhrt_kerr_emit_g(rad, ec.spin_a, kk.a2, kk.M, E, ls.lz0[lane]);
                            const int cnt = ls.cnt[lane];
                            const size_t e = (size_t)cnt * (size_t)kc.n + (size_t)i;  // k n + i
                            if (ec.out.radius) ec.out.radius[e] = rad;
                            if (ec.out.redshift) ec.out.redshift[e] = gz;
                            const double g2 = gz * gz;
                            const double w = (g2 * g2) * pow(kc.sc.disk_in / rad, ec.q);
                            ls.sum[0][lane] = ls.sum[0][lane] + w;
                            if (kc.out.rgb_r || kc.out.rgba32f || kc.out.rgba8) {
                                double br, bg, bb;
                                // (the disk colour reads sqrt(q_x^2 + q_y^2) alone)
                                colour_of(kc.sc, RAY_DISK, sqrt(sq), 0.0, 0.0, 0.0, 0.0, br, bg,
                                          bb);
                                ls.sum[1][lane] = ls.sum[1][lane] + w * br;
                                ls.sum[2][lane] = ls.sum[2][lane] + w * bg;
                                ls.sum[3][lane] = ls.sum[3][lane] + w * bb;
                            }
                            ls.cnt[lane] = cnt + 1;
                        }
                    } else {
                        rejected++;
                    }
                    if (res < 0 && steps >= kk.max_steps) res = RAY_MAX_STEPS;  // 6.
                }
                run = res < 0;
            }
        }
        if (!live) continue;
        // the tangent at the last point (as k_kerr_rk45: read from k1)
        const double tx = k1[0], ty = k1[1], tz = k1[2];
        n_rays++;
        n_steps += (unsigned)steps;
        const bhrt_frame_soa& out = kc.out;
        if (out.result) out.result[i] = res;
        if (out.steps) out.steps[i] = steps;
        if (out.hit_x) out.hit_x[i] = y[0];
        if (out.hit_y) out.hit_y[i] = y[1];
        if (out.hit_z) out.hit_z[i] = y[2];
        if (out.distance) out.distance[i] = ls.dist[lane];
        if (res == RAY_MAX_DISTANCE) {
            if (out.sky_x) out.sky_x[i] = tx;
            if (out.sky_y) out.sky_y[i] = ty;
            if (out.sky_z) out.sky_z[i] = tz;
        }
        if (kk.h_residual) kk.h_residual[i] = ls.diag[0][lane];
        if (kk.lz_drift) kk.lz_drift[i] = ls.diag[1][lane];
        if (rk.rejected) rk.rejected[i] = rejected;
        const int cnt = ls.cnt[lane];
        if (ec.out.count) ec.out.count[i] = cnt;
        if (ec.out.intensity) ec.out.intensity[i] = ls.sum[0][lane];
        if (out.rgb_r || out.rgba32f || out.rgba8) {
            double r, gg, b;
            if (cnt > 0) {
#pragma clang fp contract(off)
                r = clampd(ec.gain * ls.sum[1][lane], 0.0, 1.0);
                gg = clampd(ec.gain * ls.sum[2][lane], 0.0, 1.0);
                b = clampd(ec.gain * ls.sum[3][lane], 0.0, 1.0);
            } else {
                // the adaptive rule's colour (k_kerr_rk45's exit; a ray without crossings is
                // never RAY_DISK)
                double ut[3];
                const double t3[3] = {tx, ty, tz};
                bhrt_kerr_unit(t3, ut);
                double nv[3];
                if (camera) {
                    camera_dir(kc.cam, i % kc.cam.width, i / kc.cam.width, dir);
                } else {
                    const Ray ray = kc.rays[i];
                    dir[0] = ray.direction.x;
                    dir[1] = ray.direction.y;
                    dir[2] = ray.direction.z;
                }
                bhrt_kerr_unit(dir, nv);
                if ((kc.sc.flags & BHRT_FLAG_SKY) && res != RAY_HORIZON) {
                    const double l2 = (tx * tx + ty * ty) + tz * tz;
                    const bool take = res == RAY_MAX_DISTANCE && fabs(tx) <= kDblMax &&
                                      fabs(ty) <= kDblMax && fabs(tz) <= kDblMax && l2 > 0.0;
                    sky_lookup(kc.sky, take ? tx : nv[0], take ? ty : nv[1], take ? tz : nv[2], r,
                               gg, b);
                } else {
                    const bool tang = res == RAY_MAX_DISTANCE;
                    colour_sky(res, tang ? ut[1] : nv[1], r, gg, b);
                }
            }
            store_colour(out, i, r, gg, b);
        }
    }
    const unsigned long long s0 = wave_sum(n_rays), s1 = wave_sum(n_steps);
    if (lane == 0) {
        atomicMax(kp.ctl + 9, (unsigned long long)wall_clock64());
        if (s0) atomicAdd(kp.ctl + 1, s0);
        if (s1) atomicAdd(kp.ctl + 2, s1);
    }
}

}  // namespace

extern "C" int bhrt_launch_kerr_emit(const bhrt_kparams* kp, const bhrt_kerr_emit_k* ek,
                                     void* stream, void* ev0, void* ev1) {
    if (kp->n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    const long units =
        kp->src == BHRT_SRC_CAMERA ? (long)ek->rk.k.ntiles : ((long)kp->n + 63) / 64;
    long blocks = resident_blocks_cached<&k_kerr_emit>(64);
    if (blocks > units) blocks = units;
    if (e0) (void)hipEventRecord(e0, st);
    k_kerr_emit<<<(unsigned)blocks, 64, 0, st>>>(*kp, *ek);
    if (e1) (void)hipEventRecord(e1, st);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_kerr_rk45(const bhrt_kparams* kp, const bhrt_kerr_rk45_k* rk,
                                     void* stream, void* ev0, void* ev1) {
    if (kp->n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    const long units =
        kp->src == BHRT_SRC_CAMERA ? (long)rk->k.ntiles : ((long)kp->n + 63) / 64;
    long blocks = resident_blocks_cached<&k_kerr_rk45>(64);
    if (blocks > units) blocks = units;
    if (e0) (void)hipEventRecord(e0, st);
    k_kerr_rk45<<<(unsigned)blocks, 64, 0, st>>>(*kp, *rk);
    if (e1) (void)hipEventRecord(e1, st);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_kerr_paths(const bhrt_kparams* kp, const bhrt_kerr_paths_k* pk,
                                      void* stream, void* ev0, void* ev1) {
    if (kp->n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    const long units = ((long)kp->n + 63) / 64;
    long blocks = resident_blocks_cached<&k_kerr_paths>(64);  // one-wave workgroups (bhrt_launch.h)
    if (blocks > units) blocks = units;
    if (e0) (void)hipEventRecord(e0, st);
    k_kerr_paths<<<(unsigned)blocks, 64, 0, st>>>(*kp, *pk);
    if (e1) (void)hipEventRecord(e1, st);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_kerr(const bhrt_kparams* kp, const bhrt_kerr_k* kk, void* stream,
                                void* ev0, void* ev1) {
    if (kp->n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    const long units = kp->src == BHRT_SRC_CAMERA ? (long)kk->ntiles : ((long)kp->n + 63) / 64;
    long blocks = resident_blocks_cached<&k_kerr>(64);
    if (blocks > units) blocks = units;
    if (e0) (void)hipEventRecord(e0, st);
    k_kerr<<<(unsigned)blocks, 64, 0, st>>>(*kp, *kk);
    if (e1) (void)hipEventRecord(e1, st);
    return (int)hipGetLastError();
}
