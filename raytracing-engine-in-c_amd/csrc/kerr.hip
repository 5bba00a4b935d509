// kerr.hip -- physical geodesics of Kerr in Cartesian Kerr-Schild coordinates: four kernels for
// null rays and one for timelike particles, and their launchers.
//   k_kerr        fixed-step RK4 rays            rule: include/bhrt_api.h "Physical geodesics",
//                                                tests/kerr_rule.py; host side kerr.c
//   k_kerr_paths  the same rays' polylines       "Physical photon paths", tests/kerr_paths_rule.py;
//                                                kerr_paths.c
//   k_kerr_rk45   adaptive Dormand-Prince 5(4)   "Physical geodesics, adaptive steps",
//                                                tests/kerr_rk45_rule.py; kerr_rk45.c
//   k_kerr_emit   adaptive rays with recorded    "Kerr disk emission", tests/kerr_emit_rule.py;
//                 disk crossings                 kerr_emit.c
//   k_kerr_particles  a resident particle        "Physical particles", tests/kerr_particles_rule.py;
//                 system along timelike          kerr_particles.c. One lane per particle in 256-lane
//                 geodesics                      workgroups, on the same geom and deriv (at the end)
//
// One lane per ray, FP64. A wavefront claims 64 rays at a time from the launch's claim counter --
// an 8x8 pixel tile of a camera frame, so that its rays live alike, or 64 consecutive rays of an
// array -- and runs them until the last has ended; there is no refill of single lanes. Each stage
// forms the reciprocals of D, r, G and S once; the geometry at a step's end point serves the
// horizon test, the next step's size and the next step's first stage.
//
// Every piece of the rule stands ONCE, as a __forceinline__ function below: the claim and the
// statistics, a lane's ray and its initial data, the RK4 step and the tests after it, the
// Dormand-Prince attempt, its step factor and its Hermite disk crossing, the hit stores and the
// exit colour. A change to the rule -- the order of the tests, the 0.5 r cap, the sky rule on the exit
// direction -- is made at one place. Two exceptions, each marked where it stands: k_kerr carries
// rk4_step's text written out, because the call moved its bits, and k_kerr_rk45 carries the
// claim's, the set-up's and the exit's, because the calls cost it speed. The kernels are still four __global__ functions, one
// instantiation each, because what they keep between the pieces differs: k_kerr holds the chord and
// the diagnostics, k_kerr_paths stores points, the adaptive kernels carry k1 across attempts, and
// k_kerr_emit keeps in LDS what k_kerr_rk45 keeps in registers. Sharing the text does not share the
// register allocation: each kernel inlines the pieces into its own schedule (DESIGN.md section 17;
// profiles/kerr_shared has the resource figures and the per-kernel FP64 instruction counts, equal
// to those of the written-out loops). Within a kernel one instantiation serves camera frames and
// ray arrays, with and without a disk, a sky map or the diagnostics (wave-uniform branches outside
// the stages): a ray's arithmetic is compiled once per kernel, so its outputs are the same bits
// through every entry point. No atomic touches an output; the claim counter and the statistics are
// the only atomics.
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

// deriv at the point s, with the geometry formed there
__device__ __forceinline__ void deriv_at(const double (&s)[6], double E, const bhrt_kerr_k& k,
                                         double (&d)[6]) {
    deriv(geom(s[0], s[1], s[2], k), s[0], s[1], s[2], s[3], s[4], s[5], E, k, d);
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

// the diagnostics at an accepted point yn (before a disk hit replaces it): the largest residual so
// far and the drift of L_z from the initial data's
__device__ __forceinline__ void diag_update(const Geom& gn, const double (&yn)[6], double E,
                                            double lz0, double& hres, double& lzd) {
    hres = fmax(hres, h_residual(gn, yn, E));
    lzd = fabs((yn[0] * yn[4] - yn[1] * yn[3]) - lz0);
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

// The launch parameters as an opaque pointer into the kernel argument segment (a kernel's first
// argument starts it): the fields read through it -- the camera at a ray's set-up, the output
// pointers, the colour's constants and the sky map at its exit -- are loaded where they are used
// instead of being held in scalar registers across the steps.
typedef const __attribute__((address_space(4))) bhrt_kparams kparams_as4;
__device__ __forceinline__ const bhrt_kparams& in_kernarg(const bhrt_kparams&) {
    kparams_as4* p = (kparams_as4*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const bhrt_kparams*)p;
}

// ---- the claim and the statistics --------------------------------------------------------------

// the units of a launch: the shard's 8x8 tiles, or the 64-ray runs of an array
__host__ __device__ __forceinline__ unsigned long long kerr_units(int src, int n, int ntiles) {
    return src == BHRT_SRC_CAMERA ? (unsigned long long)ntiles
                                  : ((unsigned long long)n + 63ull) / 64ull;
}

// the wave's start stamp (ctl[8] holds the complement of the earliest)
__device__ __forceinline__ void wave_start(unsigned long long* ctl, int lane) {
    if (lane == 0) atomicMax(ctl + 8, ~(unsigned long long)wall_clock64());
}

// the wave's next unit from the claim counter ctl[0]; false once the launch's units are taken
__device__ __forceinline__ bool claim(unsigned long long* ctl, int lane, unsigned long long units,
                                      unsigned long long& unit) {
    unit = 0;
    if (lane == 0) unit = atomicAdd(ctl, 1ull);
    unit = __shfl(unit, 0);
    return unit < units;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// the wave's end stamp (ctl[9]) and its rays and steps (or attempts) into ctl[1], ctl[2]
__device__ __forceinline__ void wave_stats(unsigned long long* ctl, int lane, unsigned n_rays,
                                           unsigned n_steps) {
    const unsigned long long s0 = wave_sum(n_rays), s1 = wave_sum(n_steps);
    if (lane == 0) {
        atomicMax(ctl + 9, (unsigned long long)wall_clock64());
        if (s0) atomicAdd(ctl + 1, s0);
        if (s1) atomicAdd(ctl + 2, s1);
    }
}

// ---- a lane's ray and its initial data ---------------------------------------------------------

struct LaneRay {
    int i;      // the output element
    bool live;  // false: a lane beyond the frame's edge or the array's end (it reads ray 0)
    double o[3], dir[3];
};

// lane `lane` of 64 consecutive rays of an array
__device__ __forceinline__ LaneRay array_ray(const Ray* rays, int n, unsigned long long unit,
                                             int lane) {
    LaneRay q;
    const unsigned long long id = unit * 64ull + (unsigned)lane;
    q.live = id < (unsigned long long)n;
    q.i = (int)id;
    const Ray ray = rays[q.live ? q.i : 0];
    q.o[0] = ray.origin.x;
    q.o[1] = ray.origin.y;
    q.o[2] = ray.origin.z;
    q.dir[0] = ray.direction.x;
    q.dir[1] = ray.direction.y;
    q.dir[2] = ray.direction.z;
    return q;
}

// lane `lane` of a unit: a pixel of an 8x8 camera tile, or array_ray (kc: kp through in_kernarg)
__device__ __forceinline__ LaneRay lane_ray(const bhrt_kparams& kc, const bhrt_kerr_k& kk,
                                            bool camera, int n, unsigned long long unit, int lane) {
    if (!camera) return array_ray(kc.rays, n, unit, lane);
    LaneRay q;
    const int ty = (int)unit / kk.tiles_x, tx = (int)unit - ty * kk.tiles_x;
    const int px = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
    q.live = px < kc.cam.width && j < kk.nrows;
    q.i = j * kc.cam.width + px;
    q.o[0] = kc.cam.pos[0];
    q.o[1] = kc.cam.pos[1];
    q.o[2] = kc.cam.pos[2];
    camera_dir(kc.cam, q.live ? px : 0, q.live ? j : 0, q.dir);
    return q;
}

// n of live ray i again, by lane_ray's own operations: what a kernel that does not hold n across
// its attempts reads at the ray's exit
__device__ __forceinline__ void exit_n(const bhrt_kparams& kc, bool camera, int i,
                                       double (&nv)[3]) {
    double dir[3];
    if (camera) {
        camera_dir(kc.cam, i % kc.cam.width, i / kc.cam.width, dir);
    } else {
        const Ray ray = kc.rays[i];
        dir[0] = ray.direction.x;
        dir[1] = ray.direction.y;
        dir[2] = ray.direction.z;
    }
    bhrt_kerr_unit(dir, nv);
}

// kerr_init.h's initial data of ray q: n, the state y = (x, p), E, whether the origin has a static
// observer; returns the ray's class before its first step (-1: it runs)
__device__ __forceinline__ int initial_data(const LaneRay& q, const bhrt_kerr_k& kk,
                                            double (&nv)[3], double (&y)[6], double& E,
                                            bool& observer) {
    double l0[3], p0[3], f0;
    bhrt_kerr_unit(q.dir, nv);
    observer = bhrt_kerr_origin(q.o[0], q.o[1], q.o[2], kk.a, kk.a2, kk.two_m, kk.r_plus, &f0,
                                l0) != 0;
    bhrt_kerr_photon(f0, l0, nv, p0, &E);
    y[0] = q.o[0];
    y[1] = q.o[1];
    y[2] = q.o[2];
    y[3] = p0[0];
    y[4] = p0[1];
    y[5] = p0[2];
    return observer ? (kk.max_steps > 0 ? -1 : (int)RAY_MAX_STEPS) : (int)RAY_ERROR;
}

// ---- the fixed-step rule: k_kerr, k_kerr_paths -------------------------------------------------

// one RK4 step from y (geometry g) to yn; a step costs four geometry evaluations with the end
// point's, which the caller forms for the tests and the next step. k_kerr_paths calls this;
// k_kerr holds the same text written out (its comment says why): keep the two in step.
__device__ __forceinline__ void rk4_step(const Geom& g, const double (&y)[6], double E,
                                         const bhrt_kerr_k& kk, double (&yn)[6]) {
    const double h = kk.dt * fmin(1.0, fmax(g.r / kk.eight_m, 0.0625));
    const double hh = 0.5 * h;
    double k1[6], k2[6], k3[6], k4[6], s[6];
    deriv(g, y[0], y[1], y[2], y[3], y[4], y[5], E, kk, k1);
#pragma unroll
    for (int c = 0; c < 6; c++) s[c] = y[c] + hh * k1[c];
    deriv_at(s, E, kk, k2);
#pragma unroll
    for (int c = 0; c < 6; c++) s[c] = y[c] + hh * k2[c];
    deriv_at(s, E, kk, k3);
#pragma unroll
    for (int c = 0; c < 6; c++) s[c] = y[c] + h * k3[c];
    deriv_at(s, E, kk, k4);
    const double h6 = h / 6.0;
#pragma unroll
    for (int c = 0; c < 6; c++) yn[c] = y[c] + h6 * ((k1[c] + 2.0 * k2[c]) + (2.0 * k3[c] + k4[c]));
}

// z changed sign, or reached zero, from zo to zn
__device__ __forceinline__ bool crosses_plane(double zo, double zn) {
    return (zo > 0.0 && zn <= 0.0) || (zo < 0.0 && zn >= 0.0);
}

// The tests after step number `steps` from y to yn (geometry gn), in the rule's order; returns the
// ray's class, -1 while it runs. A disk hit replaces yn[0..2] by the hit point; `ch` gets the chord
// and `dist` grows. `accepted` runs once a finite yn is known, before a hit replaces it.
template <class F>
__device__ __forceinline__ int rk4_tests(const bhrt_kerr_k& kk, const double (&y)[6],
                                         double (&yn)[6], const Geom& gn, int steps, double& dist,
                                         double (&ch)[3], F&& accepted) {
    ch[0] = yn[0] - y[0];
    ch[1] = yn[1] - y[1];
    ch[2] = yn[2] - y[2];
    const double seg = sqrt((ch[0] * ch[0] + ch[1] * ch[1]) + ch[2] * ch[2]);
    const double zo = y[2], zn = yn[2];
    int res = -1;
    if (!finite6(yn)) return RAY_ERROR;  // 1. a non-finite state
    accepted();
    if (kk.has_disk && crosses_plane(zo, zn)) {
        const double t = zo / (zo - zn);  // 2. the disk
        const double qx = y[0] + t * ch[0], qy = y[1] + t * ch[1];
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
    return res;
}

// ---- the adaptive rule: k_kerr_rk45, k_kerr_emit -----------------------------------------------

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

// an attempt's size: the controller's, and no attempt leaps the hole
__device__ __forceinline__ double attempt_size(double hnext, const Geom& g) {
    return fmin(hnext, 0.5 * g.r);
}

// One Dormand-Prince 5(4) attempt of size h from y, whose stage 1 is k1 (FSAL: the accepted point's
// stage 7, kept across attempts): stages 2..7, the new point yn with its geometry gn and stage k7,
// and the error norm err = max_c |e_c| / (tol (1 + max(|y_c|, |ynew_c|))),
// e = h sum (b5 - b4)_j k_j
// (err_nan: a quotient was NaN, which fmax would drop). Six geometry and derivative evaluations.
// To keep what is live across the stages small -- the adaptive kernels use every register of their
// two-wave bound -- the sums of ynew and e over stages 1..5 are formed with stage 6's point, in the
// rule's order, so that k2..k5 end there.
__device__ __forceinline__ double dp_attempt(const double (&y)[6], const double (&k1)[6], double h,
                                             double E, const bhrt_kerr_k& kk, double tol,
                                             double (&yn)[6], Geom& gn, double (&k7)[6],
                                             bool& err_nan) {
    double k2[6], k3[6], k4[6], k5[6], k6[6], s[6];
#pragma unroll
    for (int c = 0; c < 6; c++) s[c] = y[c] + h * (kA21 * k1[c]);
    deriv_at(s, E, kk, k2);
#pragma unroll
    for (int c = 0; c < 6; c++) s[c] = y[c] + h * (kA31 * k1[c] + kA32 * k2[c]);
    deriv_at(s, E, kk, k3);
#pragma unroll
    for (int c = 0; c < 6; c++) s[c] = y[c] + h * ((kA41 * k1[c] + kA42 * k2[c]) + kA43 * k3[c]);
    deriv_at(s, E, kk, k4);
#pragma unroll
    for (int c = 0; c < 6; c++)
        s[c] = y[c] + h * (((kA51 * k1[c] + kA52 * k2[c]) + kA53 * k3[c]) + kA54 * k4[c]);
    deriv_at(s, E, kk, k5);
    double bs[6], es[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        s[c] = y[c] + h * ((((kA61 * k1[c] + kA62 * k2[c]) + kA63 * k3[c]) +
                            kA64 * k4[c]) + kA65 * k5[c]);
        bs[c] = ((kB1 * k1[c] + kB3 * k3[c]) + kB4 * k4[c]) + kB5 * k5[c];
        es[c] = ((kE1 * k1[c] + kE3 * k3[c]) + kE4 * k4[c]) + kE5 * k5[c];
    }
    deriv_at(s, E, kk, k6);
#pragma unroll
    for (int c = 0; c < 6; c++) {
        yn[c] = y[c] + h * (bs[c] + kB6 * k6[c]);
        es[c] = es[c] + kE6 * k6[c];
    }
    gn = geom(yn[0], yn[1], yn[2], kk);
    deriv(gn, yn[0], yn[1], yn[2], yn[3], yn[4], yn[5], E, kk, k7);
    double err = 0.0;
    err_nan = false;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double e = h * (es[c] + kE7 * k7[c]);
        const double q = fabs(e) / (tol * (1.0 + fmax(fabs(y[c]), fabs(yn[c]))));
        err_nan = err_nan || q != q;
        err = fmax(err, q);
    }
    return err;
}

// the factor of the next attempt's size after a finite err
__device__ __forceinline__ double step_factor(double err) {
    double fac = fmin(5.0, fmax(0.2, 0.9 * pow(err, -0.2)));
    if (!(fabs(fac) <= kDblMax)) fac = 0.2;
    return fac;
}

// Where an accepted attempt of size h from y to yn crosses z = 0, on the step's cubic Hermite
// polynomials q(th) = q_old + th (m0 + th (c2 + th c3)) between the tangents k1 and k7: four
// Newton iterations from the chord's crossing, kept within [0, 1].
struct Crossing {
    double m0[3], c2[3], c3[3];
    double th, qx, qy, s2;  // the parameter, the point (z = 0) and q_x^2 + q_y^2

    // the ray ends at the crossing: yn becomes the point and k7, the next k1, carries the
    // Hermite tangent there out
    __device__ __forceinline__ void end_ray(double (&yn)[6], double (&k7)[6]) const {
        yn[0] = qx;
        yn[1] = qy;
        yn[2] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) k7[c] = m0[c] + th * (2.0 * c2[c] + th * (3.0 * c3[c]));
    }
};

__device__ __forceinline__ Crossing hermite_crossing(double h, const double (&y)[6],
                                                     const double (&yn)[6],
                                                     const double (&k1)[6],
                                                     const double (&k7)[6]) {
    Crossing x;
    const double d3[3] = {yn[0] - y[0], yn[1] - y[1], yn[2] - y[2]};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x.m0[c] = h * k1[c];
        const double m1 = h * k7[c];
        x.c2[c] = (3.0 * d3[c] - 2.0 * x.m0[c]) - m1;
        x.c3[c] = (x.m0[c] + m1) - 2.0 * d3[c];
    }
    const double zo = y[2], zn = yn[2];
    double th = zo / (zo - zn);
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const double pz = zo + th * (x.m0[2] + th * (x.c2[2] + th * x.c3[2]));
        const double dz = x.m0[2] + th * (2.0 * x.c2[2] + th * (3.0 * x.c3[2]));
        const double tn = th - pz / dz;
        if (fabs(tn) <= kDblMax) th = fmin(1.0, fmax(0.0, tn));
    }
    x.th = th;
    x.qx = y[0] + th * (x.m0[0] + th * (x.c2[0] + th * x.c3[0]));
    x.qy = y[1] + th * (x.m0[1] + th * (x.c2[1] + th * x.c3[1]));
    x.s2 = x.qx * x.qx + x.qy * x.qy;
    return x;
}

// ---- a ray's exit ------------------------------------------------------------------------------

// the hit record of ray i; `sky`: the exit chord (k_kerr) or tangent (the adaptive kernels),
// stored for RAY_MAX_DISTANCE rays alone
__device__ __forceinline__ void store_hit(const bhrt_frame_soa& out, const bhrt_kerr_k& kk, int i,
                                          int res, int steps, const double (&y)[6], double dist,
                                          const double (&sky)[3], double hres, double lzd) {
    if (out.result) out.result[i] = res;
    if (out.steps) out.steps[i] = steps;
    if (out.hit_x) out.hit_x[i] = y[0];
    if (out.hit_y) out.hit_y[i] = y[1];
    if (out.hit_z) out.hit_z[i] = y[2];
    if (out.distance) out.distance[i] = dist;
    if (res == RAY_MAX_DISTANCE) {
        if (out.sky_x) out.sky_x[i] = sky[0];
        if (out.sky_y) out.sky_y[i] = sky[1];
        if (out.sky_z) out.sky_z[i] = sky[2];
    }
    if (kk.h_residual) kk.h_residual[i] = hres;
    if (kk.lz_drift) kk.lz_drift[i] = lzd;
}

__device__ __forceinline__ bool wants_colour(const bhrt_frame_soa& out) {
    return out.rgb_r || out.rgba32f || out.rgba8;
}

// The colour of a ray of class res that ended at (hx, hy, .) with exit direction t, the last chord
// (k_kerr) or the tangent at the last point (the adaptive kernels); n is its initial direction.
// With a sky map, a ray that is neither a disk hit nor in the hole looks up t if it left the scene
// and t counts (finite, squared length > 0), else n. Inlined here, not colour_of_sky's call: that
// function returns through memory. Without one, colour_of reads the unit of t -- the Doppler
// direction of a disk hit, and what the gradient reads for a ray that left the scene -- and n for
// every other ray.
__device__ __forceinline__ void exit_colour(const bhrt_kparams& kc, int res, double hx, double hy,
                                            const double (&nv)[3], const double (&t)[3],
                                            double& r, double& g, double& b) {
    double ut[3];
    bhrt_kerr_unit(t, ut);
    if ((kc.sc.flags & BHRT_FLAG_SKY) && res != RAY_DISK && res != RAY_HORIZON) {
        const double l2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
        const bool take = res == RAY_MAX_DISTANCE && fabs(t[0]) <= kDblMax &&
                          fabs(t[1]) <= kDblMax && fabs(t[2]) <= kDblMax && l2 > 0.0;
        sky_lookup(kc.sky, take ? t[0] : nv[0], take ? t[1] : nv[1], take ? t[2] : nv[2], r, g, b);
    } else {
        const bool exit_dir = res == RAY_DISK || res == RAY_MAX_DISTANCE;
        colour_of(kc.sc, res, hx, hy, exit_dir ? ut[0] : nv[0], exit_dir ? ut[1] : nv[1],
                  exit_dir ? ut[2] : nv[2], r, g, b);
    }
}

// ---- the kernels -------------------------------------------------------------------------------

// Fixed-step RK4 on (x, p), no LDS. The diagnostics are a wave-uniform branch outside the stages.
__global__ __launch_bounds__(64) void k_kerr(const bhrt_kparams kp, const bhrt_kerr_k kk) {
    const int lane = threadIdx.x;
    const bhrt_kparams& kc = in_kernarg(kp);
    const bool camera = kp.src == BHRT_SRC_CAMERA;
    const bool diag = kk.h_residual != nullptr || kk.lz_drift != nullptr;
    const unsigned long long units = kerr_units(kp.src, kp.n, kk.ntiles);
    wave_start(kp.ctl, lane);
    unsigned n_rays = 0, n_steps = 0;
    for (unsigned long long unit; claim(kp.ctl, lane, units, unit);) {
        const LaneRay q = lane_ray(kc, kk, camera, kp.n, unit, lane);
        double nv[3], y[6], E;
        bool observer;
        int res = initial_data(q, kk, nv, y, E, observer);
        int steps = 0;
        double dist = 0.0, ch[3] = {0.0, 0.0, 0.0};  // the distance, the last step's chord
        Geom g = geom(y[0], y[1], y[2], kk);
        const double lz0 = y[0] * y[4] - y[1] * y[3];
        double hres = 0.0, lzd = 0.0;
        if (diag && observer) hres = h_residual(g, y, E);
        bool run = q.live && res < 0;
        while (__ballot(run) != 0ull) {
            if (run) {
                // rk4_step's text, written out: called as the function, the stages compile to the
                // same FP64 instruction counts but another choice of which product of an
                // a*b + c*d is fused, and this kernel's hit points are no longer the bits they
                // were (profiles/kerr_shared/bitexact.txt). A change to rk4_step is made here too.
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
                const Geom gn = geom(yn[0], yn[1], yn[2], kk);
                res = rk4_tests(kk, y, yn, gn, steps, dist, ch, [&] {
                    if (diag) diag_update(gn, yn, E, lz0, hres, lzd);
                });
#pragma unroll
                for (int c = 0; c < 6; c++) y[c] = yn[c];
                g = gn;
                run = res < 0;
            }
        }
        if (!q.live) continue;
        n_rays++;
        n_steps += (unsigned)steps;
        store_hit(kc.out, kk, q.i, res, steps, y, dist, ch, hres, lzd);
        if (wants_colour(kc.out)) {
            double r, gg, b;
            exit_colour(kc, res, y[0], y[1], nv, ch, r, gg, b);
            store_colour(kc.out, q.i, r, gg, b);
        }
    }
    wave_stats(kp.ctl, lane, n_rays, n_steps);
}

// The recorded polylines of a ray array: k_kerr's rays and k_kerr's step and tests, without
// colour, sky map or diagnostics, and with the point stores.
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
    const unsigned long long units = kerr_units(BHRT_SRC_RAYS, kp.n, 0);
    wave_start(kp.ctl, lane);
    unsigned n_rays = 0, n_steps = 0;
    for (unsigned long long unit; claim(kp.ctl, lane, units, unit);) {
        const LaneRay q = array_ray(kp.rays, kp.n, unit, lane);
        const size_t row = (size_t)(q.live ? q.i : 0) * P;  // element index of the ray's slot 0
        double nv[3], y[6], E;
        bool observer;
        int res = initial_data(q, kk, nv, y, E, observer);
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
        if (q.live) emit();  // q_0, the origin as given; max_positions >= 1
        bool run = q.live && res < 0;
        while (__ballot(run) != 0ull) {
            if (run) {
                double yn[6], ch[3];
                rk4_step(g, y, E, kk, yn);
                steps++;
                const Geom gn = geom(yn[0], yn[1], yn[2], kk);
                res = rk4_tests(kk, y, yn, gn, steps, dist, ch, [] {});
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
        if (!q.live) continue;
        n_rays++;
        n_steps += (unsigned)steps;
        if (pk.out.count) pk.out.count[q.i] = (int)slot;
    }
    wave_stats(kp.ctl, lane, n_rays, n_steps);
}

// The adaptive rays: k_kerr's shape -- the claim, the set-up, the outputs, the colour, the
// statistics -- around Dormand-Prince attempts. FSAL: k1 and g are the accepted point's stage 7 and
// geometry, kept across attempts (a rejected attempt keeps them). Lanes of a wave take different
// numbers of attempts and wait for the longest; there is no refill of single lanes.
// Occupancy: two waves per SIMD, 256 registers per lane, no scratch. To fit them, n is formed again
// at the ray's exit and the exit tangent is read from k1 (DESIGN.md section 18,
// profiles/kerr_shared/resource_usage.txt).
// The attempt, the step factor and the Hermite crossing are the shared functions. The claim, the
// set-up and the exit are the shared functions' text WRITTEN OUT (wave_start / claim / wave_stats,
// lane_ray / initial_data, store_hit / exit_n / exit_colour): through the calls this kernel
// measured 0.45-0.75% slower at tolerance 1e-8 than before the pieces were shared, beyond the run-to-run
// spread, with its FP64 instruction counts unchanged; with this text it is within
// (profiles/kerr_shared/ab_parent_vs_new.txt). A change to one of those functions is made here too.
constexpr int kRk45Waves = 2;

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
        // the lane's ray: id i (the output element), origin and direction (lane_ray's text)
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
                const double h = attempt_size(hnext, g);
                double yn[6], k7[6];
                Geom gn;
                bool err_nan;
                const double err = dp_attempt(y, k1, h, E, kk, rk.tol, yn, gn, k7, err_nan);
                steps++;
                if (!finite6(yn) || err_nan || !(err <= kDblMax)) {  // 1. a non-finite attempt
                    res = RAY_ERROR;
#pragma unroll
                    for (int c = 0; c < 6; c++) y[c] = yn[c];
                } else {
                    hnext = h * step_factor(err);
                    if (err <= 1.0) {  // accepted; a rejected attempt goes to test 6 alone
                        if (diag) diag_update(gn, yn, E, lz0, hres, lzd);
                        const double cx = yn[0] - y[0], cy = yn[1] - y[1], cz = yn[2] - y[2];
                        const double seg = sqrt((cx * cx + cy * cy) + cz * cz);
                        if (kk.has_disk && crosses_plane(y[2], yn[2])) {  // 3. the disk
                            const Crossing x = hermite_crossing(h, y, yn, k1, k7);
                            if (kk.disk_lo <= x.s2 && x.s2 <= kk.disk_hi) {
                                res = RAY_DISK;
                                dist += x.th * seg;
                                x.end_ray(yn, k7);
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
            double ut[3];
            const double t3[3] = {tx, ty, tz};
            bhrt_kerr_unit(t3, ut);
            // n again, by the set-up's own operations: not held across the attempts
            double nv[3], dn[3];
            if (camera) {
                camera_dir(kc.cam, i % kc.cam.width, i / kc.cam.width, dn);
            } else {
                const Ray ray = kc.rays[i];
                dn[0] = ray.direction.x;
                dn[1] = ray.direction.y;
                dn[2] = ray.direction.z;
            }
            bhrt_kerr_unit(dn, nv);
            double r, gg, b;
            if ((kc.sc.flags & BHRT_FLAG_SKY) && res != RAY_DISK && res != RAY_HORIZON) {
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

// Disk emission: k_kerr_rk45's attempts, tests and exit, with the disk test recording up to K
// crossings per ray instead of ending the ray on its first: each crossing's radius and redshift
// (kerr_emit.h) are stored where the crossing is found -- after the attempt's state update, outside
// the stages, and rare. k_kerr_rk45 uses every register of its two-wave bound, so nothing of the
// emission is held in registers across the stages: the count, the intensity sum and the three
// colour sums wait in LDS between crossings, and so does what a ray touches once per accepted
// attempt at the most (L_z of the initial data, the distance, the two diagnostics); 76 bytes per
// lane, each lane its own words: no barrier. That is what keeps this a kernel of its own beside
// k_kerr_rk45. Two waves per SIMD, 256 registers, no scratch (DESIGN.md section 19,
// profiles/kerr_shared/resource_usage.txt).
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
    const unsigned long long units = kerr_units(kp.src, kp.n, kk.ntiles);
    wave_start(kp.ctl, lane);
    unsigned n_rays = 0, n_steps = 0;
    for (unsigned long long unit; claim(kp.ctl, lane, units, unit);) {
        const LaneRay q = lane_ray(kc, kk, camera, kp.n, unit, lane);
        const int i = q.i;
        double y[6], E;
        bool observer;
        int res;
        {
            double nv[3];  // (not held across the attempts: exit_n)
            res = initial_data(q, kk, nv, y, E, observer);
        }
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
        bool run = q.live && res < 0;
        while (__ballot(run) != 0ull) {
            if (run) {
                const double h = attempt_size(hnext, g);
                double yn[6], k7[6];
                Geom gn;
                bool err_nan;
                const double err = dp_attempt(y, k1, h, E, kk, rk.tol, yn, gn, k7, err_nan);
                steps++;
                if (!finite6(yn) || err_nan || !(err <= kDblMax)) {  // 1. a non-finite attempt
                    res = RAY_ERROR;
#pragma unroll
                    for (int c = 0; c < 6; c++) y[c] = yn[c];
                } else {
                    hnext = h * step_factor(err);
                    if (err <= 1.0) {  // accepted; a rejected attempt goes to test 6 alone
                        if (diag)
                            diag_update(gn, yn, E, ls.lz0[lane], ls.diag[0][lane],
                                        ls.diag[1][lane]);
                        const double cx = yn[0] - y[0], cy = yn[1] - y[1], cz = yn[2] - y[2];
                        const double seg = sqrt((cx * cx + cy * cy) + cz * cz);
                        bool crossed = false;  // (q_x^2 + q_y^2 of the crossing waits in LDS)
                        if (kk.has_disk && crosses_plane(y[2], yn[2])) {  // 3. the disk
                            const Crossing x = hermite_crossing(h, y, yn, k1, k7);
                            if (kk.disk_lo <= x.s2 && x.s2 <= kk.disk_hi) {
                                // crossing number cnt (the K-th ends the ray); it is recorded
                                // below, once the attempt's stage vectors are dead
                                crossed = true;
                                ls.sq[lane] = x.s2;
                                if (ls.cnt[lane] + 1 == ec.max_crossings) {
                                    res = RAY_DISK;
                                    ls.dist[lane] = ls.dist[lane] + x.th * seg;
                                    x.end_ray(yn, k7);
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
                            if (wants_colour(kc.out)) {
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
        if (!q.live) continue;
        // the tangent at the last point (as k_kerr_rk45: read from k1)
        const double tg[3] = {k1[0], k1[1], k1[2]};
        n_rays++;
        n_steps += (unsigned)steps;
        store_hit(kc.out, kk, i, res, steps, y, ls.dist[lane], tg, ls.diag[0][lane],
                  ls.diag[1][lane]);
        if (rk.rejected) rk.rejected[i] = rejected;
        const int cnt = ls.cnt[lane];
        if (ec.out.count) ec.out.count[i] = cnt;
        if (ec.out.intensity) ec.out.intensity[i] = ls.sum[0][lane];
        if (wants_colour(kc.out)) {
            double r, gg, b;
            if (cnt > 0) {
#pragma clang fp contract(off)
                r = clampd(ec.gain * ls.sum[1][lane], 0.0, 1.0);
                gg = clampd(ec.gain * ls.sum[2][lane], 0.0, 1.0);
                b = clampd(ec.gain * ls.sum[3][lane], 0.0, 1.0);
            } else {
                // the adaptive rule's colour. A ray without crossings is never RAY_DISK, so
                // colour_of is colour_sky here and the disk colour is not compiled a second time
                __builtin_assume(res != RAY_DISK);
                double nv[3];
                exit_n(kc, camera, i, nv);
                exit_colour(kc, res, y[0], y[1], nv, tg, r, gg, b);
            }
            store_colour(kc.out, i, r, gg, b);
        }
    }
    wave_stats(kp.ctl, lane, n_rays, n_steps);
}

// ---- timelike geodesics of resident particle systems: k_kerr_particles --------------------------

// One stage of the particle rule at s = (x, p, tau) with geometry g: d(x, p)/dt = (xdot, pdot) /
// tdot and dtau/dt = 1 / tdot with tdot = E + f u, its reciprocal formed once. Returns tdot.
__device__ __forceinline__ double particle_stage(const Geom& g, const double (&s)[7], double E,
                                                 const bhrt_kerr_k& k, double (&d)[7]) {
    double xp[6];
    deriv(g, s[0], s[1], s[2], s[3], s[4], s[5], E, k, xp);
    const double u = E + ((g.lx * s[3] + g.ly * s[4]) + g.lz * s[5]);
    const double tdot = E + g.f * u;
    const double it = 1.0 / tdot;
#pragma unroll
    for (int c = 0; c < 6; c++) d[c] = xp[c] * it;
    d[6] = it;
    return tdot;
}

__device__ __forceinline__ double particle_stage_at(const double (&s)[7], double E,
                                                    const bhrt_kerr_k& k, double (&d)[7]) {
    return particle_stage(geom(s[0], s[1], s[2], k), s, E, k, d);
}

// |((p.p - E^2) - f u^2) + 1| / (((E^2 + p.p) + f u^2) + 1): 2H + 1 of a unit-mass particle
__device__ __forceinline__ double particle_residual(const Geom& g, const double (&y)[7],
                                                    double E) {
    const double u = E + ((g.lx * y[3] + g.ly * y[4]) + g.lz * y[5]);
    const double pp = (y[3] * y[3] + y[4] * y[4]) + y[5] * y[5];
    const double fu2 = g.f * (u * u);
    return fabs(((pp - E * E) - fu2) + 1.0) / (((E * E + pp) + fu2) + 1.0);
}

// particles.hip's block_count, which the resident object's extract relies on: the workgroup's
// count of set flags into block_active[blockIdx.x]. Every lane of the workgroup calls it.
__device__ __forceinline__ void particles_block_count(bool active, int* block_active) {
    __shared__ int wave_count[4];
    const unsigned long long m = __ballot(active);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0)
        block_active[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

// THE PARTICLE RULE for particle i: loaded once, `steps` ticks in registers, stored once if it
// ran; returns its active flag after the call. Lanes of a wave take different numbers of substeps
// per tick (1 to 16 times pk.substeps) and wait for the longest: one flat loop over substeps, a
// tick begun where a lane's count runs out, so that lanes in different ticks still step together.
__device__ __forceinline__ int kerr_particle(Particle* ps, int i, const bhrt_kerr_particles_k& pk,
                                             int steps) {
    const bhrt_kerr_k& kk = pk.k;
    const bool diag = kk.h_residual != nullptr;
    Particle p = ps[i];
    int status = BHRT_PSTAT_INACTIVE, nsub = 0;
    double hres = 0.0, lzd = 0.0;
    if (p.active) {
        double f0, l0[3], p0[3], E, ut;
        const double v0[3] = {p.velocity.x, p.velocity.y, p.velocity.z};
        const double r0 = bhrt_kerr_fields(p.position.x, p.position.y, p.position.z, kk.a, kk.a2,
                                           kk.two_m, &f0, l0);
        if (r0 <= kk.r_plus) {  // inside the horizon at the start: the flag alone is written
            status = BHRT_PSTAT_CAPTURED;
            p.active = 0;
            ps[i].active = 0;
        } else if (!bhrt_kerr_particle(f0, l0, v0, p0, &E, &ut)) {
            status = BHRT_PSTAT_NOT_TIMELIKE;
        } else {
            status = BHRT_PSTAT_MOVED;
            double y[7] = {p.position.x, p.position.y, p.position.z, p0[0], p0[1], p0[2], 0.0};
            Geom g = geom(y[0], y[1], y[2], kk);
            const double lz0 = y[0] * y[4] - y[1] * y[3];
            if (diag) hres = particle_residual(g, y, E);
            int tick = 0, left = 0;
            double h = 0.0;
            for (;;) {
                if (left == 0) {  // a tick begins: m substeps of dt / m, m from r here
                    if (tick == steps) break;
                    tick++;
                    const double q = fmin(1.0, fmax(g.r / kk.eight_m, 0.0625));
                    left = pk.substeps * (int)ceil(1.0 / q);
                    h = kk.dt / (double)left;
                    p.age += kk.dt;
                    p.coordinate_time += kk.dt;
                }
                const double hh = 0.5 * h;
                double k1[7], k2[7], k3[7], k4[7], s[7], yn[7];
                (void)particle_stage(g, y, E, kk, k1);
#pragma unroll
                for (int c = 0; c < 7; c++) s[c] = y[c] + hh * k1[c];
                (void)particle_stage_at(s, E, kk, k2);
#pragma unroll
                for (int c = 0; c < 7; c++) s[c] = y[c] + hh * k2[c];
                (void)particle_stage_at(s, E, kk, k3);
#pragma unroll
                for (int c = 0; c < 7; c++) s[c] = y[c] + h * k3[c];
                (void)particle_stage_at(s, E, kk, k4);
                const double h6 = h / 6.0;
#pragma unroll
                for (int c = 0; c < 7; c++)
                    yn[c] = y[c] + h6 * ((k1[c] + 2.0 * k2[c]) + (2.0 * k3[c] + k4[c]));
                nsub++;
                left--;
                bool finite = true;
#pragma unroll
                for (int c = 0; c < 7; c++) finite = finite && fabs(yn[c]) <= kDblMax;
                if (!finite) {  // 1. the state before this substep stays
                    status = BHRT_PSTAT_ERROR;
                    p.active = 0;
                    break;
                }
                g = geom(yn[0], yn[1], yn[2], kk);
#pragma unroll
                for (int c = 0; c < 7; c++) y[c] = yn[c];
                if (diag) hres = fmax(hres, particle_residual(g, y, E));
                if (g.r <= kk.r_plus) {  // 2. captured at that point
                    status = BHRT_PSTAT_CAPTURED;
                    p.active = 0;
                    break;
                }
            }
            double d[7];
            const double tdot = particle_stage(g, y, E, kk, d);
            const double lz = y[0] * y[4] - y[1] * y[3];
            lzd = fabs(lz - lz0);
            p.position.x = y[0];
            p.position.y = y[1];
            p.position.z = y[2];
            p.velocity.x = d[0];
            p.velocity.y = d[1];
            p.velocity.z = d[2];
            p.energy = E;
            p.angular_momentum = lz;
            p.proper_time += y[6];
            p.time_dilation = tdot;
            ps[i] = p;
        }
    }
    if (kk.h_residual) kk.h_residual[i] = hres;
    if (kk.lz_drift) kk.lz_drift[i] = lzd;
    if (pk.status) pk.status[i] = status;
    if (pk.substeps_out) pk.substeps_out[i] = nsub;
    return p.active;
}

// One lane per particle in 256-lane workgroups, the particle index blockIdx.x * 256 + threadIdx.x:
// the layout of the resident object's per-workgroup active counts (particles.hip), which this
// kernel leaves as the parity update's counting kernel does. Lanes past count add 0 and stay for
// the barrier. FP64, no atomic.
__global__ __launch_bounds__(256) void k_kerr_particles(Particle* ps, int count,
                                                        const bhrt_kerr_particles_k pk, int steps,
                                                        int* block_active) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int active = 0;
    if (i < count) active = kerr_particle(ps, i, pk, steps);
    particles_block_count(active != 0, block_active);
}

// One launch: as many one-wave workgroups as are resident at once (bhrt_launch.h), at most one
// per unit, with ev0 / ev1 recorded around the kernel; 0 or a hipError_t value.
template <auto KERNEL, class Arg>
int launch(const bhrt_kparams* kp, const Arg* arg, long units, void* stream, void* ev0,
           void* ev1) {
    if (kp->n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    long blocks = resident_blocks_cached<KERNEL>(64);
    if (blocks > units) blocks = units;
    if (e0) (void)hipEventRecord(e0, st);
    KERNEL<<<(unsigned)blocks, 64, 0, st>>>(*kp, *arg);
    if (e1) (void)hipEventRecord(e1, st);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int bhrt_launch_kerr_particles(Particle* d, int count, const bhrt_kerr_particles_k* k,
                                          int steps, int* d_block_active, void* stream, void* ev0,
                                          void* ev1) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ev0) (void)hipEventRecord(static_cast<hipEvent_t>(ev0), st);
    if (count > 0 && steps > 0)
        k_kerr_particles<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(d, count, *k, steps,
                                                                         d_block_active);
    if (ev1) (void)hipEventRecord(static_cast<hipEvent_t>(ev1), st);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_kerr_emit(const bhrt_kparams* kp, const bhrt_kerr_emit_k* ek,
                                     void* stream, void* ev0, void* ev1) {
    const long units = (long)kerr_units(kp->src, kp->n, ek->rk.k.ntiles);
    return launch<&k_kerr_emit>(kp, ek, units, stream, ev0, ev1);
}

extern "C" int bhrt_launch_kerr_rk45(const bhrt_kparams* kp, const bhrt_kerr_rk45_k* rk,
                                     void* stream, void* ev0, void* ev1) {
    const long units = (long)kerr_units(kp->src, kp->n, rk->k.ntiles);
    return launch<&k_kerr_rk45>(kp, rk, units, stream, ev0, ev1);
}

extern "C" int bhrt_launch_kerr_paths(const bhrt_kparams* kp, const bhrt_kerr_paths_k* pk,
                                      void* stream, void* ev0, void* ev1) {
    const long units = (long)kerr_units(BHRT_SRC_RAYS, kp->n, 0);
    return launch<&k_kerr_paths>(kp, pk, units, stream, ev0, ev1);
}

extern "C" int bhrt_launch_kerr(const bhrt_kparams* kp, const bhrt_kerr_k* kk, void* stream,
                                void* ev0, void* ev1) {
    const long units = (long)kerr_units(kp->src, kp->n, kk->ntiles);
    return launch<&k_kerr>(kp, kk, units, stream, ev0, ev1);
}
