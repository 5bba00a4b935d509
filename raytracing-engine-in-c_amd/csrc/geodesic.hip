// geodesic.hip -- MI355X (gfx950) kernels of the geodesic ray tracer.
//
// One lane = one ray, FP64 throughout, the integrated state in VGPRs. What each lane
// computes is the reference's integrate_photon_path / trace_ray (src/raytracer.c:338-767,
// with rk4_integrate / rkf45_integrate of src/math_util.c:162-457 inlined), reproduced with
// its quirks: the index-shifted ray_derivatives (raytracer.c:44-154), the clamps, the
// radius step schedule and the zero-acceleration "Kerr" branch. See DESIGN.md section 2.
//
// Restructurings that leave every pinned output unchanged:
//   * trace_ray stores the whole path and scans it for the first disk crossing afterwards
//     (raytracer.c:698-759); here each segment is tested as soon as it exists and the lane
//     stops at the first hit.
//   * RKF45 never adapts h (raytracer.c:556-571 recomputes it from r), so a rejected attempt
//     leaves the state at a fixed point that rejects until max_steps; the lane jumps there.
//   * derivatives[6..7] are never written by the reference (uninitialised malloc); they are 0
//     here, so state[6..7] are per-ray constants.
//
// Divergence: rays live from 1 to max_steps iterations. The grid is persistent; every
// wavefront keeps 64 rays in flight and, once `refill` of its lanes have finished, claims
// that many new ray indices from a global queue with ONE atomic and initialises them in
// the idle lanes (ballot + popcount + lane rank), so a long ray never holds 63 idle lanes.
//
// Arithmetic: FP contraction on; quotients as a * RN(1/b) without the
// generic fdiv scaffolding; sincos specialised for the loop's argument range, shifted by angle
// addition between RK stages and carried from one iteration to the next. The hot
// instantiation contains no call: rays that need a large-argument sincos are re-traced by a
// second launch (k_trace HUGE=true).
//
// This file holds only the shipped variant. The A/B alternatives measured against it (OCML
// sincos, exact quotients, unfolded forms, per-iteration trig, the shift-statistics and
// wave-tail instrumentation) are in git history up to f099035 (tools/build_rev.sh builds any
// revision for a same-box A/B); DESIGN.md section 6 records what each was worth.
// Here: the trace path (k_init, k_trace, k_colour). The device core is bhrt_trace_core.h; k_path and
// k_paths are in paths.hip, the frame passes in frames.hip, the k_check_* kernels in checks.hip.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bhrt_kernel.h"
#include "bhrt_launch.h"

#pragma clang fp contract(fast)

namespace {

#include "bhrt_trace_core.h"

// hoist_sums: the stage sums of components 0..2 from the ray's constant state[3..5]
template <int METHOD>
__device__ __forceinline__ void zero_sums(Ray_& R) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double v = R.y[3 + i];
        if (METHOD == INTEGRATOR_RK4) {
            double a = v;
            a = rk4_acc(a, v);
            a = rk4_acc(a, v);
            R.zs[i] = a + v;
        } else {
            R.zs[i] = rkf45_sum4(v, v, v, v);
            R.zs[3 + i] = rkf45_sum5(v, v, v, v, v);
        }
    }
}

// A ray's initial state from the k_init table. A camera frame's table holds only what differs
// between its rays (BHRT_INIT_FIELDS_CAMERA rows: 64 B per ray instead of 168); the shared
// origin -- state[0..3], its Cartesian point and the sin/cos of its angles -- comes from the
// launch's camera block (wave-uniform).
__device__ __forceinline__ void load_init(const bhrt_kparams& kp, int i, Ray_& R) {
    const double* f = kp.init;
    const long n = kp.n;
    if (kp.src == BHRT_SRC_CAMERA) {
        const bhrt_camera_k& cm = kp.cam;
        R.y[0] = 0.0;
        R.y[1] = cm.r0;
        R.y[2] = cm.th0;
        R.y[3] = cm.ph0;
        R.y[4] = f[i];
        R.y[5] = f[n + i];
        R.y6 = f[2 * n + i];
        R.y7 = f[3 * n + i];
        R.dx = f[4 * n + i];
        R.dy = f[5 * n + i];
        R.dz = f[6 * n + i];
        R.far_ok = f[7 * n + i] != 0.0;
        R.px = cm.p0[0];
        R.py = cm.p0[1];
        R.pz = cm.p0[2];
        R.s1 = cm.s_r0;
        R.c1 = cm.c_r0;
        R.s2 = cm.st;
        R.c2 = cm.ct;
        R.s3 = cm.sp;
        R.c3 = cm.cp;
        R.dist = 0.0;
        R.k = 0;
        return;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) R.y[j] = f[j * n + i];
    R.y6 = f[6 * n + i];
    R.y7 = f[7 * n + i];
    R.dx = f[8 * n + i];
    R.dy = f[9 * n + i];
    R.dz = f[10 * n + i];
    R.px = f[11 * n + i];
    R.py = f[12 * n + i];
    R.pz = f[13 * n + i];
    R.far_ok = f[14 * n + i] != 0.0;
    R.s1 = f[15 * n + i];
    R.c1 = f[16 * n + i];
    R.s2 = f[17 * n + i];
    R.c2 = f[18 * n + i];
    R.s3 = f[19 * n + i];
    R.c3 = f[20 * n + i];
    R.dist = 0.0;
    R.k = 0;
}

// store_hit, and unless the launch takes the separate colour pass (colour_fused, bhrt_kernel.h)
// the colour outputs from the exit state in registers.
// The launch parameters as an opaque pointer into the kernel argument segment: the fields read
// through it are loaded (scalar loads) where they are used, instead of being kept live across
// the persistent loop. The refill's camera constants and the store's output pointers held that
// way overflowed the 106 SGPRs into VGPR lanes (v_readlane in every block of the loop).
typedef const __attribute__((address_space(4))) bhrt_kparams kparams_as4;
// (k_trace's only argument: it starts the kernel argument segment)
__device__ __forceinline__ const bhrt_kparams& cold(const bhrt_kparams&) {
    kparams_as4* p = (kparams_as4*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const bhrt_kparams*)p;
}

// SKY (a launch with a sky map; kp is cold(kp), so the map's fields are loaded here, at the exit,
// and hold no registers across the loop): the colour through colour_of_sky, or -- separate colour
// pass -- a RAY_MAX_DISTANCE ray's chord into the launch scratch for k_colour.
template <bool DISK, bool SKY = false>
__device__ __forceinline__ void store_ray(const bhrt_kparams& kp, int i, const Ray_& R, int term,
                                          const Chord& ch) {
    store_hit(kp.out, i, R, term, kp.sc);
    if constexpr (SKY) {
        if (!(kp.out.rgb_r || kp.out.rgba32f || kp.out.rgba8)) return;
        if (!kp.colour_fused) {
            if (term == T_MAXDIST && kp.sky.chord) {
                const size_t n = (size_t)kp.n;
                double cx, cy, cz;
                exit_chord(ch, R.px, R.py, R.pz, cx, cy, cz);
                kp.sky.chord[i] = cx;
                kp.sky.chord[n + i] = cy;
                kp.sky.chord[2 * n + i] = cz;
            }
            return;
        }
        const int res = term == T_DISK      ? RAY_DISK
                        : term == T_HORIZON ? RAY_HORIZON
                        : term == T_MAXDIST ? RAY_MAX_DISTANCE
                                            : RAY_MAX_STEPS;
        double r, g, b, cx, cy, cz;
        exit_chord(ch, R.px, R.py, R.pz, cx, cy, cz);  // (read for RAY_MAX_DISTANCE alone)
        colour_of_sky<DISK>(kp.sc, kp.sky, res, R.px, R.py, R.dx, R.dy, R.dz, cx, cy, cz, r, g, b);
        store_colour(kp.out, i, r, g, b);
        return;
    }
    if (kp.colour_fused && (kp.out.rgb_r || kp.out.rgba32f || kp.out.rgba8)) {
        const int res = term == T_DISK ? RAY_DISK : (term == T_HORIZON ? RAY_HORIZON : RAY_MAX_STEPS);
        double r, g, b;
        if constexpr (DISK)
            colour_of(kp.sc, res, R.px, R.py, R.dx, R.dy, R.dz, r, g, b);
        else  // (no disk: no disk colour code in the kernel)
            colour_sky(res, R.dy, r, g, b);
        store_colour(kp.out, i, r, g, b);
    }
}

// Queue position -> ray id of a camera launch: the caller's permutation (bhrt_set_claim_order),
// else the shard's pixels tile by tile -- 64-pixel tiles (8x8, 16x4 or 32x2, whichever divides
// the shard; bhrt_api.c claim_tiles), so a wavefront's rays are a compact patch of the image with
// alike lifetimes (its lanes drain together, and a frame's last rays are short tiles, not long
// row segments: claim-order probe, profiles/r03_claim_order_tiles.txt) -- else id order. Which
// lane traces a ray never changes its arithmetic, so the frame is bit-identical in every order.
__device__ __forceinline__ int claim_ray(const bhrt_kparams& kp, int qpos) {
    if (kp.order) return kp.order[qpos];
    const bhrt_camera_k& cm = kp.cam;
    if (cm.tiles_per_row == 0) return qpos;
    int t = qpos >> 6;
    const int w = qpos & 63;
    if (cm.tile_stride > 0)
        t = (int)(((unsigned long long)(unsigned)t * (unsigned)cm.tile_stride) % (unsigned)cm.ntiles);
    const int trow = div_floor(t, cm.tiles_per_row, cm.inv_tiles_per_row);
    const int tcol = t - trow * cm.tiles_per_row;
    const int prow = (trow << cm.tile_h_log2) + (w >> cm.tile_w_log2);
    const int pcol = (tcol << cm.tile_w_log2) + (w & ((1 << cm.tile_w_log2) - 1));
    return prow * cm.width + pcol;
}

// Per-ray set-up pass (integrate_photon_path's prologue, raytracer.c:355-507) into the state
// table the trace kernel refills from ([BHRT_INIT_FIELDS][n] for ray arrays; for a camera frame
// only the BHRT_INIT_FIELDS_CAMERA rows that differ between rays, 64 B per ray). Kept out of the
// persistent loop so that neither the camera uniforms nor acos/atan2 occupy registers there.
template <int SRC>
__global__ __launch_bounds__(256) void k_init(const bhrt_kparams kp) {
    double* f = kp.init;
    const long n = kp.n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kp.n; i += gridDim.x * blockDim.x) {
        Ray_ R;
        if constexpr (SRC == BHRT_SRC_CAMERA) {  // the per-ray part only (load_init)
            // row i of the table is the i-th ray of the claim order
            ray_init_camera(R, kp.cam, claim_ray(kp, i));
            f[i] = R.y[4];
            f[n + i] = R.y[5];
            f[2 * n + i] = R.y6;
            f[3 * n + i] = R.y7;
            f[4 * n + i] = R.dx;
            f[5 * n + i] = R.dy;
            f[6 * n + i] = R.dz;
            f[7 * n + i] = R.far_ok ? 1.0 : 0.0;
        } else {
            Ray ray;
            if (kp.rays_shared) {  // the origin block's point, the packed or AoS direction
                const double* d = kp.dirs + (size_t)i * kp.dir_stride;
                ray.origin = Vector3D{kp.cam.pos[0], kp.cam.pos[1], kp.cam.pos[2]};
                ray.direction = Vector3D{d[0], d[1], d[2]};
            } else {
                ray = kp.rays[i];
            }
            ray_init_general(R, 0.0, ray.origin.x, ray.origin.y, ray.origin.z, ray.direction.x,
                             ray.direction.y, ray.direction.z, kp.sc);
#pragma unroll
            for (int j = 0; j < 6; j++) f[j * n + i] = R.y[j];
            f[6 * n + i] = R.y6;
            f[7 * n + i] = R.y7;
            f[8 * n + i] = R.dx;
            f[9 * n + i] = R.dy;
            f[10 * n + i] = R.dz;
            f[11 * n + i] = R.px;
            f[12 * n + i] = R.py;
            f[13 * n + i] = R.pz;
            f[14 * n + i] = R.far_ok ? 1.0 : 0.0;
            trig_anchor(R);
            f[15 * n + i] = R.s1;
            f[16 * n + i] = R.c1;
            f[17 * n + i] = R.s2;
            f[18 * n + i] = R.c2;
            f[19 * n + i] = R.s3;
            f[20 * n + i] = R.c3;
        }
    }
}

// Per-instantiation occupancy target (waves per SIMD; 0 = the compiler's choice), same-box
// A/B in profiles/r01_ab_v11_occupancy.txt:
//  * RK4, a = 0 (C1, C2): 4. The straight-line iteration needs <= 123 VGPRs; the register
//    peak (160) sits in the rare-lane blocks (literal accelerations, wide trig shifts,
//    stores). Capped at 128 the allocator spills only inside those blocks -- the hot blocks
//    are instruction-for-instruction the 3-wave code -- so C2 gains the 4th wave (+4.6%).
//  * RKF45, a != 0, no disk (C5): 4. Since v23's two attempts per loop trip, 5 waves spill
//    (96 VGPRs + 156 B scratch) and 4 waves is best: +8.5% over 5, 6 loses 27%
//    (profiles/r02_ab_v23_occupancy.txt).
//  * C3 (RKF45 a = 0 disk): 3 (round 5: 168 VGPRs without spills), with launches of two waves
//    per SIMD (trace_launch_waves). C4 (RK4 Kerr disk) keeps the compiler's choice: 5 waves
//    spill (96 VGPRs + 84 B scratch) and gain nothing even with a capped grid.
// step sizes in VGPRs (hsel_of): the RK4 disk instantiations. C4 (Kerr, ~100 VGPRs) has the
// room; C2 (a = 0, capped at 128) gives its rare-lane blocks a few more spills but its iteration
// loses 7 v_mov_b32 (an SGPR operand of v_cndmask next to VCC exceeds gfx9's one constant-bus
// read, so each select first copied its SGPR half into a VGPR): +1.4% / +2.5% on two boxes,
// bit-identical (profiles/r03_ab/ab_v30a.txt, ab_v30b.txt)
template <int METHOD, bool DISK, bool SPIN0>
constexpr bool hsel_vgpr() {
    return METHOD == INTEGRATOR_RK4 && DISK;
}

template <int METHOD, bool DISK, bool SPIN0>
constexpr int trace_waves() {
    return (METHOD == INTEGRATOR_RKF45 && !DISK && !SPIN0) ? 4
         : (METHOD == INTEGRATOR_RK4 && SPIN0) ? 4
         : 0;
}
// the C3 camera kernel (RKF45, a = 0, disk, in-kernel set-up, near field) at 3 waves per SIMD;
// its other instantiations (ray arrays, far field, the redo pass) keep the compiler's choice
template <int METHOD, bool DISK, bool SPIN0, bool FAR, bool HUGE, int INL>
constexpr bool c3_camera() {
    return METHOD == INTEGRATOR_RKF45 && DISK && SPIN0 && !FAR && !HUGE && INL == 1;
}
// the accept-all attempts (ACC, C5): 4 per SIMD
template <int METHOD, bool DISK, bool SPIN0, bool FAR, bool HUGE, int INL, bool ACC = false>
constexpr int trace_waves_k() {
    return ACC ? 4
         : c3_camera<METHOD, DISK, SPIN0, FAR, HUGE, INL>() ? 3 : trace_waves<METHOD, DISK, SPIN0>();
}
// Waves per SIMD ONE hot launch takes (0: every resident slot). C3 is resident at 3 waves per
// SIMD (168 VGPRs, no spills) but launches 2 per SIMD's worth: the frames in flight fill the third
// slot. A full 3-wave grid deals each wave ~10 blocks in its first (static) claim and loses 10%
// against the 2-wave kernel; the 2-of-3 grid keeps ~16 blocks per wave and gains 11.6% (C3 13.1
// -> 14.6 Grays/s same-box; 448 / 576 blocks +8% / -6%, profiles/r05/ab_occupancy_grid.txt).
// The accept-all kernel (C5) launches 3 of its 4 resident waves per SIMD: +0.5...2.5% same-box
// over three sessions at 16 attempts per trip (2, 2.5 and 3.5 waves per SIMD alike, C4 -2% at 3;
// profiles/r06/ab_kernel_knobs.txt).
template <int METHOD, bool DISK, bool SPIN0, bool FAR, int INL, bool ACC = false>
constexpr int trace_launch_waves() {
    return c3_camera<METHOD, DISK, SPIN0, FAR, false, INL>() ? 2 : ACC ? 3 : 0;
}
constexpr int BHRT_TRACE_WAVES_PER_BLOCK = 4;

// Ray queues of k_trace: 64-id block b of the launch belongs to queue b mod 2^qbits; queue q's
// j-th id and its length.
__device__ __forceinline__ unsigned queue_ray(unsigned qbits, unsigned q, unsigned j) {
    return ((j >> 6) << (6u + qbits)) | (q << 6) | (j & 63u);
}
__device__ __forceinline__ unsigned queue_size(unsigned ntotal, unsigned qbits, unsigned q) {
    const unsigned nb = ntotal >> 6, last = nb & ((1u << qbits) - 1u);
    return (((nb >> qbits) + (q < last ? 1u : 0u)) << 6) + (q == last ? (ntotal & 63u) : 0u);
}  // k_trace launches 256-lane workgroups
#define BHRT_TRACE_BOUNDS __attribute__((amdgpu_flat_work_group_size(1, 256), \
                                         amdgpu_waves_per_eu(trace_waves_k<METHOD, DISK, SPIN0, FAR, HUGE, INL, ACC>() > 0 ? trace_waves_k<METHOD, DISK, SPIN0, FAR, HUGE, INL, ACC>() : 1)))

// Diagnostic build only (make DEFS=-DBHRT_WAVE_STAMPS=1, tools/wave_stamps.py): every wave of a
// hot k_trace launch records, under the launch's control-block slot, its start and end on the
// constant 100 MHz clock, its CU, and its trips, refills, lane-iterations and rays. The shipped
// build has none of it.
#ifndef BHRT_WAVE_STAMPS
#define BHRT_WAVE_STAMPS 0
#endif
#if BHRT_WAVE_STAMPS
constexpr int kStampSlots = 64, kStampWaves = 8192, kStampWords = 8;
__device__ unsigned long long g_stamps[kStampSlots * kStampWaves * kStampWords];
#endif

// Loop iterations per trip of the persistent loop (the HUGE redo pass keeps one): RKF45 with the
// accept test 2, from same-box sweeps of 1..8 (round 2); RK4 a = 0 4 under a wave-uniform guard
// (uniform_trip; predicated, 10 measured C2 +0.3…0.5%, C1 +0.5…1% against round 2's 6 and 12 / 16
// no better, profiles/r06/ab_unroll.txt). The zero-acceleration
// paths' short iterations -- C4's RK4 step (~80 VALU) and C5's untested attempt (ACC, ~55) --
// pay the trip's own cost (the live ballot, the refill test and its scalar loads) for fewer
// instructions each: 16 per trip, C4 +2.2%, C5 +14.5% same-box against 6 / 2; the sweeps
// flatten from 12 (C5) / 16 (C4) up to 24 / 32 (profiles/r06/ab_unroll.txt).
constexpr int kUnrollZA = 16, kUnrollA0 = 4;
// The trip's later iterations under a wave-uniform guard (k_trace): RK4 a = 0 (C1, C2), whose
// predicated form copies ~12 carried values (v_mov_b64) at the end of every iteration for the
// lanes that stopped. 8 per trip gave C1 +1.2%, C2 +0.4% against the predicated 10 same-box (10
// spill: 416 B scratch, C2 -65%); with the per-ray step-size cache (hcache) shallower trips win:
// 4 per trip, C2 +1.1%, C1 +4% against 8. The zero-acceleration paths stay predicated (uniform:
// C4 -1%, C5 +-0; profiles/r06/ab_unroll.txt).
template <int METHOD, bool SPIN0>
constexpr bool uniform_trip() {
    return METHOD == INTEGRATOR_RK4 && SPIN0;
}
// Whether the instantiation deals its rays over several queues (k_trace). The RK4 a = 0 path
// (C1, C2) keeps ONE queue and claims exactly the idle lanes: its rays live up to max_steps
// iterations, so claims are rare (~30 M/s on C2) and the multi-queue refill block measured -2%
// there (its registers perturb the 4-wave hot loop; same-box A/B,
// profiles/r02_claim_sweep.txt).
template <int METHOD, bool SPIN0>
constexpr bool multi_queue() {
    return !(METHOD == INTEGRATOR_RK4 && SPIN0);
}
// The exits of a wave-uniform trip as lane masks (ray_iterate MASK): the trip's guard needs only
// "does any lane stop", so an iteration ORs the ballots of its three exit compares (SALU; a disk
// hit and a `huge` ray are marked on the step count, kStopMark, and show in the budget compare);
// the termination code -- three 32-bit selects and a compare of the code in every iteration
// before -- is formed once, on the edge the trip leaves by (exit_term), from the same compares
// of the same final values. RK4 disk instantiations only (every iteration moves, so there is no
// fixed-point exit). The reference's exit order and every output are unchanged.
template <int METHOD, bool DISK, bool SPIN0>
constexpr bool exit_masks() {
    return uniform_trip<METHOD, SPIN0>() && DISK && METHOD == INTEGRATOR_RK4;
}
// the reference's exit order (disk, horizon, distance, step budget) after ray_iterate<MASK>,
// T_NONE for a lane that goes on; takes the disk hit's mark off the step count
__device__ __forceinline__ int exit_term(Ray_& R, const Scene& sc) {
    const bool dhit = R.k < 0;
    R.k &= ~kStopMark;
    int term = (R.k >= sc.max_steps) ? T_MAXSTEPS : T_NONE;
    term = (R.dist >= sc.max_dist) ? T_MAXDIST : term;
    term = (R.y[1] <= sc.rs_x1_05) ? T_HORIZON : term;
    return dhit ? T_DISK : term;
}
template <int METHOD, bool SPIN0, bool FAR, bool HUGE, bool ACC = false>
constexpr int unroll_n() {
    return HUGE                      ? 1
         : METHOD == INTEGRATOR_RK4  ? (zero_accel<SPIN0, FAR>() ? kUnrollZA : kUnrollA0)
         : ACC                       ? kUnrollZA
                                     : 2;
}

// Persistent trace kernel: grid = what is resident; each wave refills idle lanes from the
// global queue kp.ctl[0] (one returning atomic per refill).
// FAR: some ray may take ray_derivatives' weak-field branch (origin beyond 15 rs). A camera
// frame knows this once for all its rays (shared origin); ray arrays always assume it.
// HUGE = false: the hot instantiation, rays [0, kp.n) from the queues kp.qhead. A ray that
// needs a large-argument sincos (bhrt_sincos) is dropped and its id appended to kp.redo
// (count ctl[6]). HUGE = true: re-traces kp.redo[0, ctl[6]) from queue head ctl[7].
// INL: rays set up here, at refill, instead of being loaded from k_init's table: 1 = camera
// launch (ray_init_camera), 2 = ray array with one shared origin (ray_init_shared: the origin's
// set-up from the host, the direction from the array). Used where rays are short-lived (Kerr,
// RKF45), so refills are frequent and each table load stalls its wave on HBM latency, and on the
// a = 0 RK4 disk path; ray arrays from trace_rays_batch take 2, so a chunk's
// trace depends on its upload alone (no set-up kernel queued behind the previous chunk's).
// The sin/cos anchors of the shared origin are the same for every ray: computed once per wave.
// SKY: the launch has a sky map (kp.sky): the iterations keep their chord (ray_iterate) and the
// exit looks the map up (store_ray). Instantiated for sky launches only; every other
// instantiation is the code it was.
template <int METHOD, bool DISK, bool SPIN0, bool FAR, bool HUGE, int INL = 0, bool ACC = false,
          bool SKY = false>
__global__ BHRT_TRACE_BOUNDS void k_trace(const bhrt_kparams kp) {
    const unsigned long long total =
        HUGE ? *(volatile unsigned long long*)(kp.ctl + 6) : (unsigned long long)kp.n;
    if (total == 0) return;
    // sin, cos of the origin state's angles (r0, th0, ph0): the host's libm values
    const double as1 = kp.cam.s_r0, ac1 = kp.cam.c_r0, as2 = kp.cam.st, ac2 = kp.cam.ct,
                 as3 = kp.cam.sp, ac3 = kp.cam.cp;
    const int lane = threadIdx.x & 63;
    // the launch's execution window on the constant-rate wall clock (bhrt_stats.frame_ms:
    // first wave's start to the last wave's end, or the colour pass's end): ctl[8] holds the
    // complement of the start -- stamped by the first workgroup's first wave alone (workgroups
    // are dispatched in order; one atomic per wave at the launch's start would serialise 4096
    // atomics on one word) -- and ctl[9] the latest end
    if (!HUGE && blockIdx.x == 0 && threadIdx.x == 0)
        atomicMax(kp.ctl + 8, ~(unsigned long long)wall_clock64());
#if BHRT_WAVE_STAMPS
    const unsigned long long st_t0 = (unsigned long long)wall_clock64();
    unsigned st_trips = 0, st_refills = 0, st_claims = 0;
    unsigned long long st_claim_t = 0, st_first = 0;  // time in claim round trips; the first's
#endif
    const unsigned long long below = (1ull << lane) - 1ull;
    Counters n;
    Ray_ R;
    Chord ch{0.0, 0.0, 0.0};  // (read by the sky instantiations only)
    int rid = 0;
    bool live = false;
    // Ray queues. The rays are dealt, in blocks of 64 consecutive ids, round
    // robin over Q = 2^queue_bits queues, each with its own head word: every claim is a
    // returning device-scope atomic, and claims on ONE word serialise at the memory side
    // (~65 M/s: short-lived scenes -- C3 -- were bound by exactly that rate with one queue).
    // A wave starts on queue (its index mod Q) and moves on to the next queue when its own
    // runs dry, never back (a dry queue stays dry). A claim takes the lanes' need; with
    // claim_div > 0 it takes a block (the queue's unclaimed remainder / (waves * claim_div),
    // at least claim_min, guided scheduling) that the wave hands out over its next refills.
    // Per-wave state in LDS (touched only at refill, so it holds no registers across the
    // loop): [lo, hi) = claimed ids not yet handed out, cur = queue, moves = queues left behind.
    // (The RK4 a = 0 path keeps one queue: multi_queue.)
    constexpr bool MULTIQ = multi_queue<METHOD, SPIN0>();
    __shared__ unsigned s_q[BHRT_TRACE_WAVES_PER_BLOCK][4];
    const unsigned ntotal = (unsigned)total;
    const unsigned qbits = HUGE ? 0u : (unsigned)kp.queue_bits;
    const unsigned nq = 1u << qbits;
    unsigned long long* const heads = HUGE ? kp.ctl + 7 : kp.qhead;
    const unsigned qstride = HUGE ? 0u : (unsigned)kp.queue_stride;
    // claim = remainder >> shift (no division in the loop; claim_shift from the launcher)
    const unsigned shift = (unsigned)kp.claim_shift;
    const int wv = threadIdx.x >> 6;
    if (MULTIQ && lane == 0) {
        s_q[wv][0] = 0u;
        s_q[wv][1] = 0u;
        s_q[wv][2] = (blockIdx.x * (blockDim.x >> 6) + wv) & (nq - 1u);
        s_q[wv][3] = 0u;
    }
    // Deferred stores (drained-refill instantiations): a ray that finishes keeps its final state
    // in its lane's registers (the lane takes no new ray before the wave's next refill) and is
    // stored AT that refill, together with every other lane that finished meanwhile -- where a
    // wave refills only once drained (C3, C4, C5), all 64 lanes store at once, full lines of
    // every field, instead of a few lanes per trip (partial lines, written to HBM more than once:
    // C3's traffic was 1.40x its output) -- and the trip loop has no store code in it.
    constexpr bool DEFER = MULTIQ && !HUGE;
    int pterm = T_NONE;  // DEFER: how this lane's finished ray ended (T_NONE: nothing pending)
    bool exhausted = false;  // no ids left to claim or hand out; wave-uniform
    const HSel hsel = hsel_of<hsel_vgpr<METHOD, DISK, SPIN0>()>(kp.sc);
    for (;;) {
        // (re-laundered at the top of every trip, in wave-uniform control flow)
        const bhrt_kparams& kc = cold(kp);
        const unsigned long long live_mask = __ballot(live);
        int n_live = __popcll(live_mask);
        if (!exhausted && (64 - n_live >= kp.refill || n_live == 0)) {
#if BHRT_WAVE_STAMPS
            st_refills++;
#endif
            if constexpr (DEFER) {
                if (pterm != T_NONE) store_ray<DISK, SKY>(kc, rid, R, pterm, ch);
                pterm = T_NONE;
            }
            bool ok;
            unsigned long long id;
            if constexpr (MULTIQ) {
                const unsigned need = 64u - (unsigned)n_live;
                unsigned lo = __builtin_amdgcn_readfirstlane(s_q[wv][0]);
                unsigned hi = __builtin_amdgcn_readfirstlane(s_q[wv][1]);
                unsigned cur = __builtin_amdgcn_readfirstlane(s_q[wv][2]);
                unsigned moves = __builtin_amdgcn_readfirstlane(s_q[wv][3]);
                const unsigned avail = hi - lo;
                const unsigned rank = (unsigned)__popcll(~live_mask & below);
                unsigned q = cur, j = lo + rank;  // lanes beyond the block take ids of the new claim
                ok = rank < avail;
                if (avail >= need || moves >= nq) {
                    lo += avail >= need ? need : avail;
                } else {
                    const unsigned want = need - avail;
                    unsigned b = 0, e = 0;
                    bool hopped = false;
                    for (;;) {  // wave-uniform; ends once a claim lands or every queue is dry
                        const unsigned size = queue_size(ntotal, qbits, cur);
                        unsigned long long* const hp = heads + (size_t)cur * qstride;
                        unsigned c = want;
                        if (kp.claim_div > 0 && !hopped) {
                            c = ((size - hi) >> shift) + 63u & ~63u;
                            if (c < (unsigned)kp.claim_min) c = (unsigned)kp.claim_min;
                            if (c < want) c = want;
                        }
                        unsigned long long base = 0;
#if BHRT_WAVE_STAMPS
                        const unsigned long long tq0 = (unsigned long long)wall_clock64();
#endif
                        if (lane == 0) base = atomicAdd(hp, (unsigned long long)c);
                        base = __shfl(base, 0);
#if BHRT_WAVE_STAMPS
                        {
                            const unsigned long long dtq = (unsigned long long)wall_clock64() - tq0;
                            st_claim_t += dtq;
                            if (st_claims++ == 0) st_first = dtq;
                        }
#endif
                        if (base < size) {
                            b = (unsigned)base;
                            e = base + c < size ? (unsigned)(base + c) : size;
                            break;
                        }
                        // Queue `cur` is dry. The queues not yet left behind are looked at in
                        // ONE round trip -- lane k reads the head of queue cur + 1 + k -- and
                        // the wave moves to the first with ids left (a dry queue stays dry).
                        // Hopping one queue per round trip had cost a wave up to 15 serial
                        // atomic round trips (~30 us) at the end of every launch: a quarter of a
                        // strong-scaled C4 shard's wave lifetime (tools/wave_stamps.py).
                        const unsigned left = nq - 1u - moves;
                        bool room = false;
                        if ((unsigned)lane < left) {
                            const unsigned qk = (cur + 1u + (unsigned)lane) & (nq - 1u);
                            room = __hip_atomic_load(heads + (size_t)qk * qstride, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT) <
                                   (unsigned long long)queue_size(ntotal, qbits, qk);
                        }
                        const unsigned long long rm = __ballot(room);
                        if (rm == 0ull) {
                            moves = nq;
                            break;
                        }
                        const unsigned k = (unsigned)__builtin_ctzll(rm);
                        moves += k + 1u;
                        cur = (cur + 1u + k) & (nq - 1u);
                        hi = 0u;
                        hopped = true;
                    }
                    if (!ok) {
                        q = cur;
                        j = b + (rank - avail);
                        ok = j < e;
                    }
                    lo = b + want < e ? b + want : e;
                    hi = e;
                }
                exhausted = moves >= nq && lo >= hi;
                if (lane == 0) {
                    s_q[wv][0] = lo;
                    s_q[wv][1] = hi;
                    s_q[wv][2] = cur;
                    s_q[wv][3] = moves;
                }
                id = queue_ray(qbits, q, j);
            } else {
                const int need = 64 - n_live;
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(heads, (unsigned long long)need);
                base = __shfl(base, 0);
                exhausted = base + (unsigned long long)need >= total;
                id = base + __popcll(~live_mask & below);
                ok = id < total;
            }
            if (!live) {
                if (ok) {
                    // queue position -> ray id; the k_init table is in queue order
                    const int qpos = (int)id;
                    rid = HUGE ? kp.redo[id] : (kp.src == BHRT_SRC_CAMERA ? claim_ray(kc, qpos) : qpos);
                    // (the redo list holds ray ids; the k_init table is in claim order)
                    if (INL || (HUGE && (kp.order || kp.cam.tiles_per_row))) {
                        if constexpr (INL == 2)
                            ray_init_shared(R, kc.cam, kc.dirs, kc.dir_stride, rid);
                        else
                            ray_init_camera(R, kc.cam, rid);
                        R.s1 = as1;
                        R.c1 = ac1;
                        R.s2 = as2;
                        R.c2 = ac2;
                        R.s3 = as3;
                        R.c3 = ac3;
                    } else {
                        load_init(kp, HUGE ? rid : qpos, R);
                    }
                    // the first iteration's state recovery (the loop is skipped at max_steps <= 0);
                    // an in-kernel camera set-up has a finite origin (|r0| < 2^20, host-checked),
                    // so only the velocities can need it and the origin's sin/cos stay valid
                    if (repair_at_refill<METHOD, FAR, HUGE>() && kp.sc.max_steps > 0)
                        state_repair<!INL>(R, &n);
                    if (hoist_sums<METHOD, SPIN0, FAR, HUGE>()) zero_sums<METHOD>(R);
                    if (hcache<METHOD, SPIN0, FAR, HUGE>()) R.h_lo = R.h_hi = __builtin_nan("");  // select on entry
                    // the far-field bound (repair_at_refill) not proven for this ray: it is handed
                    // to the HUGE redo pass after its first trip, like a large-argument ray (the
                    // trip's one iteration is discarded; a branch here would cost spills at
                    // every refill)
                    if (FAR && !HUGE && !(kp.sc.far_bounded && state_within(R, 0x1p40)))
                        n.raise_huge();
                    // the rotation of state[2]'s sin, cos needs |h state[5]| < pi/4 (rotation_trig)
                    if (rotation_trig<METHOD, SPIN0, FAR, HUGE>() && !(fabs(R.y[5]) < kp.sc.rot_vmax))
                        n.raise_huge();
                    n.rays++;
                    live = true;
                    if (kp.sc.max_steps <= 0) {  // loop never runs: MAX_STEPS, steps 0
                        store_ray<DISK, SKY>(kc, rid, R, T_MAXSTEPS, ch);
                        live = false;
                        n.clear_huge();
                    }
                }
            }
            n_live = __popcll(__ballot(live));
        }
        if (n_live == 0) {
            if (exhausted) {
                if constexpr (DEFER) {
                    if (pterm != T_NONE) store_ray<DISK, SKY>(kc, rid, R, pterm, ch);
                }
                break;
            }
            continue;
        }
#if BHRT_WAVE_STAMPS
        st_trips++;
#endif
        if (live) {
            // further iterations in the same trip for rays that go on: the loop's hand-over
            // copies between iterations (state, point, distance, carried sin/cos) fold away. A
            // lane's iterations are the same either way; only its refill point moves.
            int term;
            if constexpr (exit_masks<METHOD, DISK, SPIN0>()) {
                // (the wave-uniform guard below, on the wave's exit mask)
                unsigned long long stop =
                    ray_iterate<METHOD, DISK, SPIN0, FAR, HUGE, ACC, true, SKY>(R, kp.sc, n, hsel, &ch);
#pragma unroll
                for (int u = 1; u < unroll_n<METHOD, SPIN0, FAR, HUGE, ACC>(); u++) {
                    if (stop != 0ull) break;  // (a lane that raised `huge` is marked: Counters)
                    stop = ray_iterate<METHOD, DISK, SPIN0, FAR, HUGE, ACC, true, SKY>(R, kp.sc, n, hsel, &ch);
                }
                term = T_NONE;
                if (stop != 0ull) term = exit_term(R, kp.sc);
            } else if constexpr (uniform_trip<METHOD, SPIN0>()) {
                term = ray_iterate<METHOD, DISK, SPIN0, FAR, HUGE, ACC, false, SKY>(R, kp.sc, n, hsel, &ch);
                // wave-uniform guard: the trip goes on only while EVERY live lane does, so the
                // next iteration runs on the same exec mask -- no per-lane region around it, and
                // no copies of the values a lane that stopped must keep (they are copied once, on
                // the trip's exit edge, instead of after every iteration)
#pragma unroll
                for (int u = 1; u < unroll_n<METHOD, SPIN0, FAR, HUGE, ACC>(); u++) {
                    if (__ballot(term != T_NONE || n.huge) != 0ull) break;
                    term = ray_iterate<METHOD, DISK, SPIN0, FAR, HUGE, ACC, false, SKY>(R, kp.sc, n, hsel, &ch);
                }
            } else {
                term = ray_iterate<METHOD, DISK, SPIN0, FAR, HUGE, ACC, false, SKY>(R, kp.sc, n, hsel, &ch);
#pragma unroll
                for (int u = 1; u < unroll_n<METHOD, SPIN0, FAR, HUGE, ACC>(); u++)
                    if (term == T_NONE && !n.huge)
                        term = ray_iterate<METHOD, DISK, SPIN0, FAR, HUGE, ACC, false, SKY>(R, kp.sc, n, hsel, &ch);
            }
            if (METHOD == INTEGRATOR_RK4 && (term != T_NONE || (!HUGE && n.huge)))
                n.iters += R.k;  // every RK4 iteration moves, so R.k = iterations executed
            if (!HUGE && n.huge) {  // hand the ray to the HUGE instantiation
                n.clear_huge();
                n.rays--;
                kp.redo[atomicAdd(kp.ctl + 6, 1ull)] = rid;
                // no redo pass follows a launch the host proved eviction-free: if that proof
                // was wrong for this scene, the ray is marked, never left stale (the host's
                // harvest reports the count as an error, context.c)
                if (kc.no_evict && kc.skip_redo && kc.out.result) kc.out.result[rid] = RAY_ERROR;
                live = false;
            } else if (term != T_NONE) {
                if constexpr (DEFER)
                    pterm = term;
                else
                    store_ray<DISK, SKY>(kc, rid, R, term, ch);
                live = false;
            }
        }
    }
    const unsigned long long s0 = wave_sum(n.rays), s1 = wave_sum(n.iters),
                             s3 = wave_sum(n.far_);
    unsigned long long s2, s4;
    if ((FAR && HUGE) || BHRT_COUNT_STAGES) {  // stages counted one by one
        s2 = wave_sum(n.full);
        s4 = wave_sum(n.kerr);
    } else {  // every stage that was not a far-field one took the instantiation's branch
        const unsigned long long st =
            s1 * (METHOD == INTEGRATOR_RK4 ? 4ull : (METHOD == INTEGRATOR_RKF45 ? 6ull : 0ull)) -
            (FAR ? s3 : 0ull);
        s2 = SPIN0 ? st : 0ull;
        s4 = SPIN0 ? 0ull : st;
    }
#if BHRT_WAVE_STAMPS
    if (!HUGE && lane == 0 && kp.diag_slot >= 0 && kp.diag_slot < kStampSlots) {
        const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        if (w < (unsigned)kStampWaves) {
            unsigned long long* p =
                g_stamps + ((size_t)kp.diag_slot * kStampWaves + w) * kStampWords;
            p[0] = st_t0;
            p[1] = (unsigned long long)wall_clock64();
            p[2] = (unsigned long long)__smid();
            p[3] = (unsigned long long)st_trips | ((unsigned long long)st_refills << 32);
            p[4] = s1;
            p[5] = s0;
            p[6] = st_claim_t | ((unsigned long long)st_claims << 48);
            p[7] = st_first;
        }
    }
#endif
    if (lane == 0) {
        atomicMax(kp.ctl + 9, (unsigned long long)wall_clock64());
        if (s0) atomicAdd(kp.ctl + 1, s0);
        if (s1) atomicAdd(kp.ctl + 2, s1);
        if (s2) atomicAdd(kp.ctl + 3, s2);
        if (s3) atomicAdd(kp.ctl + 4, s3);
        if (s4) atomicAdd(kp.ctl + 5, s4);
    }
}

// SKY: a sky launch's pass (its own instantiation: the plain pass keeps its registers)
template <int SRC, bool SKY = false>
__global__ __launch_bounds__(256) void k_colour(const bhrt_kparams kp) {
    const bhrt_frame_soa& s = kp.out;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kp.n; i += gridDim.x * blockDim.x) {
        double dx, dy, dz;
        if (SRC == BHRT_SRC_CAMERA) {
            camera_dir(kp.cam, i, dx, dy, dz);
        } else if (kp.rays_shared) {
            const double* d = kp.dirs + (size_t)i * kp.dir_stride;
            dx = d[0];
            dy = d[1];
            dz = d[2];
        } else {
            dx = kp.rays[i].direction.x;
            dy = kp.rays[i].direction.y;
            dz = kp.rays[i].direction.z;
        }
        const int res = s.result[i];
        double r, g, b;
        const double hx = res == RAY_DISK ? s.hit_x[i] : 0.0, hy = res == RAY_DISK ? s.hit_y[i] : 0.0;
        if constexpr (SKY) {  // the chords of the launch's RAY_MAX_DISTANCE rays are in the scratch
            const size_t n = (size_t)kp.n;
            const bool md = res == RAY_MAX_DISTANCE && kp.sky.chord;
            colour_of_sky<true>(kp.sc, kp.sky, res, hx, hy, dx, dy, dz, md ? kp.sky.chord[i] : 0.0,
                                md ? kp.sky.chord[n + i] : 0.0, md ? kp.sky.chord[2 * n + i] : 0.0,
                                r, g, b);
        } else {
            colour_of(kp.sc, res, hx, hy, dx, dy, dz, r, g, b);
        }
        store_colour(s, i, r, g, b);
    }
    __syncthreads();  // the frame is complete once the last workgroup's stores are (ctl[10])
    if (threadIdx.x == 0) atomicMax(kp.ctl + 10, (unsigned long long)wall_clock64());
}

// smallest shift with 2^shift >= (waves * claim_div) / 2^queue_bits, at least 1 (a grid of
// fewer waves than queues claims half a queue's remainder at a time); 0 = exact claims
int claim_shift(int blocks, int claim_div, int queue_bits, int lanes = 256) {
    if (claim_div <= 0) return 0;
    const unsigned long long wq =
        ((unsigned long long)blocks * (unsigned)(lanes / 64) * (unsigned)claim_div) >> queue_bits;
    int shift = 1;
    while (shift < 31 && (1ull << shift) < wq) shift++;
    return shift;
}

template <int METHOD, bool DISK, bool SPIN0, bool FAR, int INL, bool ACC, bool SKY>
void launch_trace_pair_t(const bhrt_kparams& kp, hipStream_t st) {
    // resident workgroups of the two instantiations, per device (and per hot block size:
    // kp.block_lanes, 64/128/256 lanes -- a workgroup's slot frees only once ALL its waves
    // have drained, so small launches prefer one wave per workgroup)
    static std::atomic<int> grid_cap[kMaxDev][3], grid_huge[kMaxDev];
    const int dev = current_device();
    const int lanes = kp.block_lanes == 64 || kp.block_lanes == 128 ? kp.block_lanes : 256;
    const int bi = lanes == 64 ? 0 : lanes == 128 ? 1 : 2;
    int cap = grid_cap[dev][bi].load(std::memory_order_relaxed);
    int cap_huge = grid_huge[dev].load(std::memory_order_relaxed);
    if (cap == 0 || cap_huge == 0) {
        cap = resident_blocks(
            reinterpret_cast<const void*>(&k_trace<METHOD, DISK, SPIN0, FAR, false, INL, ACC, SKY>), dev,
            lanes);
        cap_huge = resident_blocks(
            reinterpret_cast<const void*>(&k_trace<METHOD, DISK, SPIN0, FAR, true, INL, false, SKY>), dev);
        grid_cap[dev][bi].store(cap, std::memory_order_relaxed);
        grid_huge[dev].store(cap_huge, std::memory_order_relaxed);
    }
    int blocks = (kp.n + lanes - 1) / lanes;
    // Waves of a drained-refill launch (C3, C4, C5) get their work in guided blocks whose first
    // claim is the queue's size / its waves, so a launch of few tiles per wave is partitioned
    // almost statically at its start and ends with the waves that drew the costliest tiles
    // (a strong-scaled C4 shard: ~4 tiles per wave, trips per wave from 12 to 46,
    // profiles/r05/c4_shard_wave_stamps.txt). Such a launch -- fewer than min_tiles 64-ray
    // tiles per wave on the resident grid -- takes half the grid and shares the chip with the
    // next frames' launches: C4 8-GPU shard 0.146 -> 0.127 ms, 4-GPU shard +3.6% same-box,
    // while launches of >= 16 tiles per wave lose 6-7% at half the grid (C3, C4 full, C5) and a
    // quarter grid loses against a half (profiles/r05/ab_grid_fraction.txt, ab_min_tiles.txt).
    // kp.grid_div > 0 overrides (BHRT_GRID_DIV).
    if (trace_launch_waves<METHOD, DISK, SPIN0, FAR, INL, ACC>() > 0 && kp.grid_blocks <= 0) {
        const int lw = device_cus(dev) * trace_launch_waves<METHOD, DISK, SPIN0, FAR, INL, ACC>() * 4 / (lanes / 64);
        if (lw > 0 && lw < cap) cap = lw;
    }
    if (kp.grid_blocks > 0) {  // (A/B: an absolute grid, BHRT_GRID_BLOCKS)
        cap = kp.grid_blocks < cap ? kp.grid_blocks : cap;
    } else if (kp.grid_div > 0) {
        cap = cap / kp.grid_div > 0 ? cap / kp.grid_div : 1;
    } else if (multi_queue<METHOD, SPIN0>() && kp.min_tiles > 0 &&
               (long)kp.n < 64L * kp.min_tiles * (long)cap * (lanes / 64)) {
        cap = (cap + 1) / 2;
    }
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    bhrt_kparams k = kp;
    k.claim_shift = claim_shift(blocks, kp.claim_div, kp.queue_bits, lanes);
    k_trace<METHOD, DISK, SPIN0, FAR, false, INL, ACC, SKY><<<blocks, lanes, 0, st>>>(k);
    // A launch the host proved eviction-free (scene.c origin_no_evict: every ray starts at
    // one origin, and every state the loop can reach keeps its sincos arguments below 2^20 --
    // C1, C2, C3 -- or, on the zero-acceleration paths, C4 and C5, the loop has no sincos and
    // the one refill-time test |state[5]| < rot_vmax holds for every unit direction) hands no
    // ray over: no redo launch follows, one dispatch less per frame, and the frame's end no
    // longer waits behind the next frame's persistent workgroups for a wave slot
    if (kp.no_evict && kp.skip_redo) return;
    // rays evicted by the large-argument check (normally none: every wave exits at once). 64
    // workgroups: the evicted rays are rare, and a full-chip grid of waves that only read the
    // count and exit costs ~15 us per frame (C3 +8.5% same-box, profiles/r02_ab_v24.txt)
    // A far-field launch the host could not prove bounded hands every ray over: full grid.
    int redo_blocks = (FAR && !kp.sc.far_bounded) ? blocks : (blocks < 64 ? blocks : 64);
    if (redo_blocks > cap_huge) redo_blocks = cap_huge;
    k.claim_shift = claim_shift(redo_blocks, kp.claim_div, 0);  // (the redo list is one queue)
    k_trace<METHOD, DISK, SPIN0, FAR, true, INL, false, SKY><<<redo_blocks, 256, 0, st>>>(k);
}

// the pair of a launch: its sky instantiations where it has a sky map (bhrt_fill_scene sets
// kp.sky only with BHRT_FLAG_SKY), else the plain ones
template <int METHOD, bool DISK, bool SPIN0, bool FAR, int INL, bool ACC = false>
void launch_trace_pair(const bhrt_kparams& kp, hipStream_t st) {
    if (kp.sky.tex)
        launch_trace_pair_t<METHOD, DISK, SPIN0, FAR, INL, ACC, true>(kp, st);
    else
        launch_trace_pair_t<METHOD, DISK, SPIN0, FAR, INL, ACC, false>(kp, st);
}

template <int METHOD, bool DISK, bool SPIN0, bool FAR>
int launch_t(const bhrt_kparams& kp, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    // camera rays set up inside k_trace (no k_init table, no table load at refill): scenes with
    // a disk (most rays end on it within tens of iterations: C4 +6.6%, C3 +16.5%; the a = 0 RK4
    // path since v31, whose in-kernel set-up now fits the 4-wave 128-VGPR cap with spills only
    // in rare-lane blocks: C2 +1.2% same-box, profiles/r03_ab/ab_c2inl.txt), and the Kerr RKF45
    // path without a disk (C5: 51 attempts per ray since v21's cheaper attempts, so k_init's
    // 168-byte table -- 0.7 GB written and read per 8K shard -- outweighs the set-up: +1.5%
    // same-box, profiles/r02_ab_v20_occupancy.txt; it lost 5% on round 1's 193-attempt slab,
    // r01_ab_v10.txt).
    // Ray arrays with one shared origin (kp.rays_shared) the same way where a camera frame
    // would (mode 2: the direction from the array).
    constexpr bool CAN_INL = DISK ? true : (METHOD == INTEGRATOR_RKF45 && !SPIN0);
    const int inl = !CAN_INL || !(fabs(kp.cam.r0) < 1048576.0) ? 0
                  : kp.src == BHRT_SRC_CAMERA                  ? 1
                  : kp.rays_shared                             ? 2
                                                               : 0;
    if (inl)
        ;
    else if (kp.src == BHRT_SRC_CAMERA)
        k_init<BHRT_SRC_CAMERA><<<grid_for(reinterpret_cast<const void*>(&k_init<BHRT_SRC_CAMERA>),
                                           kp.n), 256, 0, st>>>(kp);
    else
        k_init<BHRT_SRC_RAYS><<<grid_for(reinterpret_cast<const void*>(&k_init<BHRT_SRC_RAYS>),
                                         kp.n), 256, 0, st>>>(kp);
    if (ev0) (void)hipEventRecord(ev0, st);
    // attempts that cannot be rejected (rkf45_attempt ACC): the zero-acceleration RKF45
    // instantiations with the host's accept_all (C5)
    constexpr bool CAN_ACC = METHOD == INTEGRATOR_RKF45 && accept_all_ok<SPIN0, FAR, false>();
    if constexpr (CAN_ACC && CAN_INL) {
        if (kp.sc.accept_all && inl == 1)
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 1, true>(kp, st);
        else if (kp.sc.accept_all && inl == 2)
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 2, true>(kp, st);
        else if (kp.sc.accept_all)
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 0, true>(kp, st);
        else if (inl == 1)
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 1>(kp, st);
        else if (inl == 2)
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 2>(kp, st);
        else
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 0>(kp, st);
    } else if constexpr (CAN_INL) {
        if (inl == 1)
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 1>(kp, st);
        else if (inl == 2)
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 2>(kp, st);
        else
            launch_trace_pair<METHOD, DISK, SPIN0, FAR, 0>(kp, st);
    } else {
        launch_trace_pair<METHOD, DISK, SPIN0, FAR, 0>(kp, st);
    }
    if (ev1) (void)hipEventRecord(ev1, st);
    if (!kp.colour_fused && (kp.out.rgb_r || kp.out.rgba32f || kp.out.rgba8)) {
        if (kp.sky.tex && kp.src == BHRT_SRC_CAMERA)
            k_colour<BHRT_SRC_CAMERA, true><<<grid_for(reinterpret_cast<const void*>(
                                                           &k_colour<BHRT_SRC_CAMERA, true>),
                                                       kp.n), 256, 0, st>>>(kp);
        else if (kp.sky.tex)
            k_colour<BHRT_SRC_RAYS, true><<<grid_for(reinterpret_cast<const void*>(
                                                         &k_colour<BHRT_SRC_RAYS, true>),
                                                     kp.n), 256, 0, st>>>(kp);
        else if (kp.src == BHRT_SRC_CAMERA)
            k_colour<BHRT_SRC_CAMERA><<<grid_for(reinterpret_cast<const void*>(&k_colour<BHRT_SRC_CAMERA>),
                                                 kp.n), 256, 0, st>>>(kp);
        else
            k_colour<BHRT_SRC_RAYS><<<grid_for(reinterpret_cast<const void*>(&k_colour<BHRT_SRC_RAYS>),
                                               kp.n), 256, 0, st>>>(kp);
    }
    return (int)hipGetLastError();
}

template <int METHOD, bool DISK, bool SPIN0>
int dispatch_far(const bhrt_kparams& kp, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    // a camera frame, or a ray array with one shared origin, knows from the host whether its
    // origin is beyond 15 rs (use_analytic_approx); other ray arrays assume some ray may be
    const bool far = (kp.src == BHRT_SRC_CAMERA || kp.rays_shared) ? kp.cam.use_approx != 0 : true;
    return far ? launch_t<METHOD, DISK, SPIN0, true>(kp, st, e0, e1)
               : launch_t<METHOD, DISK, SPIN0, false>(kp, st, e0, e1);
}

template <int METHOD, bool DISK>
int dispatch_spin(const bhrt_kparams& kp, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    return kp.sc.spin0 ? dispatch_far<METHOD, DISK, true>(kp, st, e0, e1)
                       : dispatch_far<METHOD, DISK, false>(kp, st, e0, e1);
}

template <int METHOD>
int dispatch_disk(const bhrt_kparams& kp, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    return kp.sc.has_disk ? dispatch_spin<METHOD, true>(kp, st, e0, e1)
                          : dispatch_spin<METHOD, false>(kp, st, e0, e1);
}

}  // namespace

extern "C" int bhrt_launch_trace(const bhrt_kparams* kp, void* stream, void* ev0, void* ev1) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    switch (kp->sc.method) {
    case INTEGRATOR_RK4: return dispatch_disk<INTEGRATOR_RK4>(*kp, st, e0, e1);
    case INTEGRATOR_RKF45: return dispatch_disk<INTEGRATOR_RKF45>(*kp, st, e0, e1);
    default: return dispatch_disk<INTEGRATOR_LEAPFROG>(*kp, st, e0, e1);  // no-op integrators
    }
}

// whether bhrt_launch_trace runs this launch's RKF45 attempts without the accept test (the
// ACC instantiations above: the host's accept_all on a zero-acceleration path), for the
// statistics' attempts_untested
extern "C" int bhrt_trace_untested(const bhrt_kparams* kp) {
    if (kp->sc.method != INTEGRATOR_RKF45 || !kp->sc.accept_all) return 0;
    const bool far = (kp->src == BHRT_SRC_CAMERA || kp->rays_shared) ? kp->cam.use_approx != 0 : true;
    if (kp->sc.spin0)
        return far ? accept_all_ok<true, true, false>() : accept_all_ok<true, false, false>();
    return far ? accept_all_ok<false, true, false>() : accept_all_ok<false, false, false>();
}

#if BHRT_WAVE_STAMPS
// Diagnostic build: copy the per-wave stamps to host memory dst (kStampSlots x kStampWaves x
// kStampWords u64; NULL = do not copy) and, with reset, zero them. Synchronises the device.
extern "C" __attribute__((visibility("default"))) long bhrt_diag_stamps(void* dst, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (dst && hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), sizeof g_stamps) != hipSuccess)
        return -1;
    if (reset) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_stamps)) != hipSuccess ||
            hipMemset(p, 0, sizeof g_stamps) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return -1;
    }
    return (long)sizeof g_stamps;
}
#endif
