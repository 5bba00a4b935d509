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
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "bhrt_kernel.h"

#pragma clang fp contract(fast)

namespace {

constexpr double kEps = 1.0e-10;  // BH_EPSILON (math_util.h:21)
constexpr double kTwoPi = 6.28318530717958647692;

using Scene = bhrt_scene_k;

// The mark ray_iterate<MASK> (k_trace's wave-uniform trip) puts on a ray's step count when the
// ray must leave the trip for a reason that is no compare of its own: a disk hit, or `huge`
// (ORed in from Counters::mark). The trip's guard then sees it in the step-budget compare
// (unsigned) instead of balloting two more lane masks.
constexpr int kStopMark = (int)0x80000000u;
struct Counters {
    unsigned rays = 0, iters = 0, full = 0, far_ = 0, kerr = 0;
    bool huge = false;  // a sincos argument needed the large-argument path (see bhrt_sincos)
    int mark = 0;       // kStopMark while `huge` is raised
    __device__ __forceinline__ void raise_huge() {
        huge = true;
        mark = kStopMark;
    }
    __device__ __forceinline__ void clear_huge() {
        huge = false;
        mark = 0;
    }
};

// Division without the generic fdiv scaffolding.
// rcp_nr is RN(1/b) for b in the normal range: v_rcp_f64 (good to ~2^-24,
// tools/probe/trans_probe.hip) and one cubically convergent step y0 (1 + e + e^2), e^3 ~ 2^-72
// far below the final rounding -- three FMAs instead of the compiler's two Newton steps. One
// reciprocal serves every quotient with the same divisor, and div_nr(a, b, rcp_nr(b)) is
// a * RN(1/b) (<= 1.5 ulp; the same order as the FMA contraction): on every BASELINE config it
// leaves the class and step of every sampled ray equal to the compiled reference's and the hit
// points as close (profiles/r01_bench_all_configs_v6.jsonl), for 7% of C2. Callers keep the
// IEEE a / b for out-of-range operands.
__device__ __forceinline__ double rcp_nr(double b) {
    const double y = __builtin_amdgcn_rcp(b);
    const double e = __builtin_fma(-b, y, 1.0);
    return __builtin_fma(y, __builtin_fma(e, e, e), y);
}
__device__ __forceinline__ double div_nr(double a, double /*b*/, double yb) { return a * yb; }
// -2 * rcp_nr(b), bit for bit: the seed is scaled by -2 (a power of two, exact) beside the
// residual, and the same refinement runs on the scaled seed, so every intermediate is rcp_nr's
// times -2 (b in the normal range, as for rcp_nr). One product off the dependent chain instead
// of the two `* -2.0` of rhs's accelerations behind it.
__device__ __forceinline__ double rcp_nr_m2(double b) {
    const double y = __builtin_amdgcn_rcp(b);
    const double e = __builtin_fma(-b, y, 1.0);
    const double y2 = y * -2.0;
    return __builtin_fma(y2, __builtin_fma(e, e, e), y2);
}

// fma(a, b, c) with c a compile-time coefficient, as ONE v_fma_f64 whose addend is an SGPR
// pair (set up by SALU). Left to itself hipcc copies the coefficient into the destination
// (v_mov_b64) and uses v_fmac_f64: two VALU instructions per Horner step.
__device__ __forceinline__ double fmac_k(double a, double b, double c) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

// max(a, b) as ONE v_max_f64 (b in SGPRs): fmax would first canonicalize both operands
// (v_max_f64 x, x, x) for its NaN rule; callers pass non-NaN a.
__device__ __forceinline__ double max_raw(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b));
    return r;
}
// max(|a|, |b|) as ONE v_max_f64 with both abs modifiers (non-NaN a, b)
__device__ __forceinline__ double max_abs_raw(double a, double b) {
    double r;
    asm("v_max_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Guards decided from the HIGH WORDS of their f64 operands. A double's high 32
// bits hold its sign, exponent and top 20 mantissa bits, so an integer operation on high words
// can FILTER for a straight-line path: it may send a lane that belongs on the fast path to the
// rare block -- which first makes the exact f64 test and sends such a lane back -- and never lets
// a lane that fails the exact test through. The results are then the exact test's, bit for bit.
// Only forms that SAVE INSTRUCTIONS are built: a 32-bit compare of one high word issues no
// faster than the f64 compare it would replace (4 cycles either way beside an f64 stream, at 1
// and at 4 waves per SIMD: tools/probe/cmp_probe.hip, profiles/guardwords/cmp_probe.txt).
// The filter is in the RK4 stage pairs (rhs_given: C2 +1.3%, C1 +1.9% same-box), not in the
// single-stage form (rhs), which RKF45 runs: there it lost 3.6% on C3 same-box, its kernel
// gaining scratch (profiles/guardwords/ab_parent_vs_new.txt).
// the high word of x: a sub-register read, no instruction
__device__ __forceinline__ unsigned hiword(double x) {
    return (unsigned)(__builtin_bit_cast(unsigned long long, x) >> 32);
}
// Filter for "a, b and c are all plain values of magnitude <= 10" (accel_fast): bit 30 of a
// high word -- the top bit of the 11-bit exponent field -- is set exactly when the double is
// NaN, +-Inf or at least 2 in magnitude (biased exponent >= 1024), so it is clear in the OR of
// the three exactly when all three are finite and below 2. Read as a float the OR has bit 30
// clear exactly when its magnitude is below 2.0f (biased exponent < 128; a NaN pattern fails the
// ordered compare as it must): one v_or3_b32 and one v_cmp_lt_f32 with the |.| modifier, where
// the exact test is three v_cmp_le_f64 and two s_and_b64. true implies the exact test passes; a
// lane with some |value| in [2, 10] gets false and is sent back by the exact test.
__device__ __forceinline__ bool all_below_2(double a, double b, double c) {
    const unsigned w = hiword(a) | hiword(b) | hiword(c);
    return __builtin_fabsf(__builtin_bit_cast(float, w)) < 2.0f;
}

// sin and cos of one argument, for the trace loop. OCML's sincos
// spends ~78 VALU per call on a range reduction valid to 2^30+; every argument here (the
// radius read as an angle by ray_derivatives, theta, phi) stays far below 2^20, where a
// three-constant Cody-Waite reduction with FMA is exact up to a double-double tail. The
// tail feeds the fdlibm kernels (k_sin.c / k_cos.c, FreeBSD form). Measured on 6e7 random
// arguments against glibc (the reference's libm): max 1 ulp, 97% bit-identical.
// |x| >= 2^20 takes OCML's sincos (not inlined: its Payne-Hanek path must not cost registers
// in the loop).
__device__ __attribute__((noinline)) void sincos_ocml(double x, double* s, double* c) {
    sincos(x, s, c);
}

// hc == nullptr: |x| >= 2^20 takes OCML's out-of-line path. Otherwise (the hot trace loop,
// which must contain no call: the call ABI would spill the ray state to scratch) a finite
// |x| >= 2^20 only raises hc->huge and the ray is re-traced by the HUGE instantiation;
// Inf and NaN need no special path (the reduction below turns them into NaN, as glibc does).
__device__ __forceinline__ void bhrt_sincos(double x, double* so, double* co,
                                            Counters* hc = nullptr) {
    if (!(fabs(x) < 1048576.0)) {
        if (!hc) {
            sincos_ocml(x, so, co);
            return;
        }
        if (fabs(x) <= 1.79769313486231570815e+308) hc->raise_huge();
    }
    constexpr double kTwoOverPi = 6.36619772367581382433e-01;
    constexpr double P1 = 1.57079632679489655800e+00;   // pi/2 in three parts
    constexpr double P2 = 6.12323399573676603587e-17;
    constexpr double P3 = -1.49738490485916983e-33;
    const double n = rint(x * kTwoOverPi);
    const double r1 = __builtin_fma(-n, P1, x);          // exact for |x| < 2^20
    const double p2 = n * P2;
    const double p2e = __builtin_fma(n, P2, -p2);        // n*P2 = p2 + p2e exactly
    const double hi = r1 - p2;                           // TwoSum(r1, -p2)
    const double t = hi - r1;
    const double e = (r1 - (hi - t)) - (p2 + t);
    const double lo = __builtin_fma(-n, P3, e - p2e);
    const double r = hi + lo;                            // reduced argument r + y
    const double y = (hi - r) + lo;
    constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                     S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                     S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                     C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                     C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = r * r, w = z * z;
    const double rs_ = fmac_k(z, fmac_k(z, S4, S3), S2) + z * w * fmac_k(z, S6, S5);
    const double v = z * r;
    const double s = r - ((z * (0.5 * y - v * rs_) - y) - v * S1);
    const double rc = z * fmac_k(z, fmac_k(z, C3, C2), C1) +
                      w * w * fmac_k(z, fmac_k(z, C6, C5), C4);
    const double hz = 0.5 * z, ww = 1.0 - hz;
    const double c = ww + (((1.0 - ww) - hz) + (z * rc - r * y));
    const int q = (int)n;
    double ss = (q & 1) ? c : s;
    double cc = (q & 1) ? s : c;
    *so = (q & 2) ? -ss : ss;
    *co = ((q + 1) & 2) ? -cc : cc;
}

// sin and cos of a + delta from s0 = sin(a), c0 = cos(a), delta in
// [-pi/4, pi/4]: sin(delta) and cos(delta) - 1 from the fdlibm k_sin / k_cos polynomials, and
// the shift adds only small corrections to s0, c0 (error <= the direct value's + 0.5 ulp).
// Returns false, leaving the outputs unset, when delta is outside [-pi/4, pi/4] or when
// a + delta - a would not be exact; the caller then evaluates sincos directly.
__device__ __forceinline__ bool sincos_shift_wide(double a, double s0, double c0, double x,
                                                  double& s, double& c) {
    const double delta = x - a;  // exact when x in [a/2, 2a] (Sterbenz)
    if (!(fabs(delta) <= 0.78539816339744828 && fabs(delta) <= 0.5 * fabs(a))) return false;
    constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                     S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                     S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                     C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                     C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = delta * delta, w = z * z;
    const double r = fmac_k(z, fmac_k(z, S4, S3), S2) + z * w * fmac_k(z, S6, S5);
    const double sd = delta + (z * delta) * fmac_k(z, r, S1);       // k_sin, tail 0
    const double rc = z * fmac_k(z, fmac_k(z, C3, C2), C1) +
                      w * w * fmac_k(z, fmac_k(z, C6, C5), C4);
    const double cm1 = z * rc - 0.5 * z;                             // k_cos - 1
    s = s0 + (s0 * cm1 + c0 * sd);
    c = c0 + (c0 * cm1 - s0 * sd);
    return true;
}

// sin(delta) and cos(delta) - 1: for |delta| <= 1/16 shift_or_eval's polynomials, above that
// (|delta| <= pi/4) the fdlibm k_sin / k_cos ones of sincos_shift_wide
__device__ __forceinline__ void rotation_coeffs(double delta, double& sd, double& cm1) {
    const double z = delta * delta;
    if (__builtin_expect(fabs(delta) <= 0.0625, 1)) {
        constexpr double S1 = -0.16666666666662605, S2 = 0.00833333327878775,
                         S3 = -0.00019839069723619096;
        constexpr double C1 = 0.04166666666666157, C2 = -0.0013888888827212717,
                         C3 = 2.479927034006378e-05;
        sd = delta + (z * delta) * fmac_k(z, fmac_k(z, S3, S2), S1);
        cm1 = z * __builtin_fma(z, fmac_k(z, fmac_k(z, C3, C2), C1), -0.5);
        return;
    }
    constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                     S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                     S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                     C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                     C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double w = z * z;
    const double r = fmac_k(z, fmac_k(z, S4, S3), S2) + z * w * fmac_k(z, S6, S5);
    sd = delta + (z * delta) * fmac_k(z, r, S1);
    const double rc = z * fmac_k(z, fmac_k(z, C3, C2), C1) + w * w * fmac_k(z, fmac_k(z, C6, C5), C4);
    cm1 = z * rc - 0.5 * z;
}

// sin, cos of x given those of a nearby a, as the trace loop needs them: every RK stage after
// the first evaluates ray_derivatives at theta = y1 + delta (the stage increment; |delta| < 0.09
// on a full C2 frame), and the three angles of the state move by one step per iteration.
// Nearly every shift is tiny (on a full C2 frame |x - a| > 0.0625 in < 0.7% of wave
// evaluations at any site), so every lane first runs polynomials fitted to |delta| <= 1/16 --
// three coefficients each for sin(delta) and cos(delta) - 1 instead of fdlibm's six, max error
// 2.4e-19 / 1.0e-21 (tools/shift_poly_fit.py) -- straight-line, and only a lane outside that
// interval then redoes the shift with sincos_shift_wide (|delta| <= pi/4) or evaluates directly.
// The choice is per lane, so a ray's rounding never depends on its wave-mates.
__device__ __forceinline__ void shift_or_eval(double a, double s0, double c0, double x, double& s,
                                              double& c, Counters* hc) {
    const double delta = x - a;  // exact when |delta| <= |a| / 2 (Sterbenz)
    constexpr double S1 = -0.16666666666662605, S2 = 0.00833333327878775,
                     S3 = -0.00019839069723619096;
    constexpr double C1 = 0.04166666666666157, C2 = -0.0013888888827212717,
                     C3 = 2.479927034006378e-05;
    const double z = delta * delta;
    const double sd = delta + (z * delta) * fmac_k(z, fmac_k(z, S3, S2), S1);  // sin(delta)
    const double cm1 = z * __builtin_fma(z, fmac_k(z, fmac_k(z, C3, C2), C1), -0.5);
    // s0 (1 + cm1) + c0 sd as two FMAs (<= 1 ulp)
    s = __builtin_fma(c0, sd, __builtin_fma(s0, cm1, s0));
    c = __builtin_fma(-s0, sd, __builtin_fma(c0, cm1, c0));
    // (delta = x - a is exact for |x - a| <= |a| / 2 (Sterbenz); otherwise -- a near 0 -- it is
    // off by <= ulp(delta) / 2 <= 3.5e-18, well below the polynomials' rounding)
    if (__builtin_expect(!(fabs(delta) <= 0.0625), 0)) {
        if (!sincos_shift_wide(a, s0, c0, x, s, c)) bhrt_sincos(x, &s, &c, hc);
    }
}

// shift_or_eval from a NEARER anchor, with shorter polynomials. Two of the RK4
// a = 0 iteration's six shifts have an angle at hand whose sin and cos are already in registers
// and that lies a SECOND-order distance from the target, where the iteration's start lies a
// first-order one (tools/shift_deltas.py; largest |eps| of a 480x270 C2 frame in brackets):
//   NC = 2  stage 3 from stage 2: theta3 - theta2 = h/2 (k2 - k1)[1]  [0.0086]: two coefficients
//           each on |eps| <= 1/64, max error 1.2e-18 / 1.7e-21 (tools/shift_poly_fit.py);
//   NC = 1  the advance of state[1] from stage 4: theta' - theta4      [0.00078]: one coefficient
//           each on |eps| <= 2^-10, max error 9.8e-19 / 1.3e-22.
// No lane of camera B's frame, or of frames from inside 15 rs off the polar axis, is beyond
// either bound, so a wave of mixed rays does not pay for the branch (what a narrower polynomial
// from the far anchor did: 0.5-0.8% of lanes beyond 1/64). Views down the polar axis, where the
// |d| <= 10 clamp binds, do have such lanes (0.5-1% beyond 1/64, 0.3-0.5% beyond 2^-10; up to
// 1.5% beyond 2^-10 from far off-axis cameras); measured on camera A's on-axis frame the short
// forms still gain 3.7% against 3.8% on camera B (profiles/shiftchain/ab_parent_vs_new.txt).
// A lane with !(|eps| <= bound) -- NaN included -- redoes the shift with shift_or_eval from the
// same anchor, whose wide and direct forms treat every operand as before. Per lane, so a ray's
// rounding never depends on its wave-mates. Returns whether the lane kept the short form.
template <int NC>
__device__ __forceinline__ bool shift_chain(double a, double s0, double c0, double x, double& s,
                                            double& c, Counters* hc) {
    static_assert(NC == 1 || NC == 2, "one coefficient on 2^-10 or two on 1/64");
    constexpr double BOUND = NC == 2 ? 0.015625 : 0.0009765625;
    const double eps = x - a;  // exact when |eps| <= |a| / 2 (Sterbenz), as in shift_or_eval
    const double z = eps * eps;
    double sd, cm1;
    if constexpr (NC == 2) {
        constexpr double S1 = -0.16666666666059188, S2 = 0.008333261288663034;
        constexpr double C1 = 0.04166666666580769, C2 = -0.001388879428493602;
        sd = eps + (z * eps) * fmac_k(z, S2, S1);
        cm1 = z * __builtin_fma(z, fmac_k(z, C2, C1), -0.5);
    } else {
        constexpr double S1 = -0.16666665974827055, C1 = 0.04166666547825309;
        sd = __builtin_fma(z * eps, S1, eps);
        cm1 = z * __builtin_fma(z, C1, -0.5);
    }
    s = __builtin_fma(c0, sd, __builtin_fma(s0, cm1, s0));
    c = __builtin_fma(-s0, sd, __builtin_fma(c0, cm1, c0));
    const bool fast = fabs(eps) <= BOUND;
    if (__builtin_expect(!fast, 0)) shift_or_eval(a, s0, c0, x, s, c, hc);
    return fast;
}

// Trig of theta (= y[1]) for one RK stage: stage 1 takes it from the previous iteration
// (carried in Ray_), later stages shift it.
struct Trig1 {
    double a, s, c;  // theta of stage 1 and its sin, cos
};

// ray_derivatives' a = 0 accelerations in the literal form (:92-130, evaluation order as
// written, divisions as div_nr / IEEE), from sin, cos of the unclamped theta.
__device__ __forceinline__ void accel_literal(const double (&y)[6], double (&d)[6], const Scene& sc,
                                              double st, double ct) {
    double r = y[0];
    double rsq = r * r;
    double st2 = st * st;
    if (r <= sc.rs_x1_5) {
        r = sc.rs_x1_5;
        rsq = r * r;
    }
    if (fabs(st) < 0.01) {
        st = (st >= 0.0) ? 0.01 : -0.01;
        st2 = st * st;
    }
    const double term2 = r * y[4] * y[4];
    const double term3 = r * st2 * y[5] * y[5];
    const double n4 = -2.0 * y[3] * y[4];
    const double n5a = -2.0 * y[3] * y[5];
    const double n5b = 2.0 * y[4] * y[5] * ct;
    const double sc4 = st * ct * y[5] * y[5];
    if (r < 1.0e150) {  // r >= 1.5 rs here: every divisor is in the normal range
        const double yr = rcp_nr(r);
        // -M / (r^2 f) * f == -M / r^2 in exact arithmetic
        const double term1 = -(sc.M * yr) * yr;
        d[3] = term1 + term2 + term3;
        d[4] = div_nr(n4, r, yr) + sc4;
        d[5] = div_nr(n5a, r, yr) - div_nr(n5b, st, rcp_nr(st));
    } else {
        const double f = 1.0 - sc.rs / r;
        const double term1 = -sc.M / (rsq * f) * f;
        d[3] = term1 + term2 + term3;
        d[4] = n4 / r + sc4;
        d[5] = n5a / r - n5b / st;
    }
}

// :141-153 -- non-finite -> 0 for all six, then |d[3..5]| <= 10. BOUNDED (k_trace's hot
// instantiations, repair_at_refill): d[0..2] are the stage state's velocities, finite there, so
// only d[3..5] are looked at -- and d[0..2] stay the very registers of the stage state (no copies)
template <bool BOUNDED = false>
__device__ __forceinline__ void repair_clamp(double (&d)[6]) {
#pragma unroll
    for (int i = BOUNDED ? 3 : 0; i < 6; i++)
        if (!isfinite(d[i])) d[i] = 0.0;
#pragma unroll
    for (int i = 3; i < 6; i++) d[i] = fmin(fmax(d[i], -10.0), 10.0);
}

// The a = 0 accelerations of one stage in the fast form, given w2 = -2 / (rc st) (rhs, which
// takes it from the stage's own reciprocal, or rk4_step's pair, which shares one between two
// stages). ok: the operands the reciprocal was taken of are in range -- |sin theta| >= 0.01 and,
// where it is tested, rc < 1e150, of this stage and of the one it shares the reciprocal with.
// A lane that fails it, or whose result is not a plain |d| <= 10 value, recomputes the stage in
// the literal form (its own reciprocals) before the repair and clamps.
template <bool HUGE, bool WORDS>
__device__ __forceinline__ void accel_fast(const double (&y)[6], double (&d)[6], const Scene& sc,
                                           double st, double ct, double rc, double w2, bool ok) {
    // The factor -2 of d4 and d5 rides on the reciprocal (w2 = -2 / (r sin theta), rcp_nr_m2):
    // yr2 = -2 / r, ys2 = -2 / sin theta and p2 = -2 v_r / r are the former yr, ys, p times a
    // power of two, so every product and FMA below rounds as before -- d4 = fma(p * -2, v_th,
    // ..), d5 = (v_ph * -2) * fma(v_th, cos th * ys, p), d3 = fma(-(M yr), yr, f3) with
    // (M / 4 * yr2) * yr2, M / 4 the host's (Scene m_4) -- bit-identical, one VALU less
    const double yr2 = st * w2, ys2 = rc * w2;
    const double u = st * y[5];
    const double f3 = rc * __builtin_fma(u, u, y[4] * y[4]);
    d[3] = __builtin_fma(-(sc.m_4 * yr2), yr2, f3);
    const double p2 = y[3] * yr2;
    d[4] = __builtin_fma(p2, y[4], u * (ct * y[5]));
    d[5] = y[5] * __builtin_fma(y[4], ct * ys2, p2);
    // WORDS: the straight-line path's guard is the high-word filter (all_below_2: 2 VALU for the
    // exact test's 3, and two scalar ANDs less); a lane it holds back -- some |d| in [2, 10], or
    // truly out of range -- takes the exact test first, in the rare block, so the lanes that go
    // on to the literal form are exactly the exact test's
    if constexpr (WORDS)
        if (__builtin_expect((int)ok & (int)all_below_2(d[3], d[4], d[5]), 1)) return;
    const int plain = (int)ok & (int)(fabs(d[3]) <= 10.0) & (int)(fabs(d[4]) <= 10.0) &
                      (int)(fabs(d[5]) <= 10.0);
    if (__builtin_expect(plain, 1)) return;
    accel_literal(y, d, sc, st, ct);
    repair_clamp<!HUGE>(d);
}

// ray_derivatives (raytracer.c:44-154) for one RK stage. y = (t, r, theta, phi, tdot, rdot)
// of the caller, read -- as the reference does -- as (r, theta, phi, v_r, v_theta, v_phi).
// Stage counters: FAR instantiations count their far-field stages (a lane's branch varies);
// every other stage takes the instantiation's one other branch, and k_trace derives that count
// from the iterations (the HUGE redo, whose RKF45 attempts can stop after stage 1, counts
// every stage).
// Stage-counting build (make DEFS=-DBHRT_COUNT_STAGES=1 -> diag/libbhrt_count.so, built by
// __graft_entry__.build()): every instantiation counts each stage's branch one by one, as the
// FAR && HUGE redo pass always does, instead of deriving the split from the iterations -- the
// GPU test test_stage_counts_are_counted checks that both give the same counters (the FLOP
// credit of bench.py rests on the derived ones) and the same frame.
#ifndef BHRT_COUNT_STAGES
#define BHRT_COUNT_STAGES 0
#endif
template <bool SPIN0, bool FAR, bool HUGE>
__device__ __forceinline__ void rhs(const double (&y)[6], double (&d)[6], const Scene& sc,
                                    bool far_ok, Counters& n, Trig1& tr, bool first) {
    d[0] = y[3];
    d[1] = y[4];
    d[2] = y[5];
    if (FAR && far_ok && y[0] > sc.rs_x15) {  // weak-field branch, no NaN/clamp pass (:65-86)
        d[3] = 0.0;
        d[4] = 0.0;
        d[5] = y[5] * (sc.two_m / (y[0] * y[0]));
        n.far_++;
        return;
    }
    if (SPIN0) {  // :92-130
        double st, ct;
        if (first) {
            st = tr.s;  // carried from the previous iteration (ray_iterate)
            ct = tr.c;
        } else {
            shift_or_eval(tr.a, tr.s, tr.c, y[1], st, ct, HUGE ? nullptr : &n);
        }
        if ((FAR && HUGE) || BHRT_COUNT_STAGES) n.full++;
        // Fast form, straight-line: the same three accelerations with the divisions as one
        // reciprocal and the products regrouped -- d3 = -M/r^2 + r (v_th^2 + (sin th v_ph)^2),
        // d4 = -2 v_r v_th / r + (sin th v_ph)(cos th v_ph),
        // d5 = -2 v_ph (v_r / r + v_th cos th / sin th) -- a few ulp from the literal
        // expressions. y[0] is finite (the state is repaired before
        // the first iteration or at the top of every iteration, and a stage adds a bounded
        // increment), so fmax is the reference's clamp. A lane whose result is not a plain
        // |d| <= 10 value, or whose |sin theta| < 0.01 clamp would bind (never on a C2 frame),
        // recomputes it in the literal form before the repair and clamps.
        const double rc = max_raw(y[0], sc.rs_x1_5);
        // 1/r and 1/sin theta from one reciprocal of the product (r sin theta in [0.03, 1e150]):
        // one v_rcp_f64 + refinement fewer per stage, <= ~2 ulp instead of 1 (+1.7% at 4 waves)
        // rc < 1e150 (every divisor of the literal form normal) needs no test in k_trace's hot
        // instantiations: state[0] starts at t = 0 there and moves by h * state[3], whose own
        // derivative is the clamped |d3| <= 10 (or 0), so |state[0]| <= 0.1 * 20 * steps^2;
        // k_path (a caller-given t) and the HUGE redo keep it
        const bool ok = (!HUGE ? true : rc < 1.0e150) & (fabs(st) >= 0.01);
        // (no high-word filter here: it lost 3.6% on C3, see all_below_2)
        accel_fast<HUGE, false>(y, d, sc, st, ct, rc, rcp_nr_m2(rc * st), ok);
        return;
    }
    // :131-138
    d[3] = 0.0;
    d[4] = 0.0;
    d[5] = 0.0;
    if ((FAR && HUGE) || BHRT_COUNT_STAGES) n.kerr++;
    // Far-field and Kerr stages: the repair / clamps never change a value here but run as the
    // reference's pass whenever a component is not a plain |d| <= 10 value (NaN and Inf fail
    // the test). d[0..2] = y[3..5] need no test: the iteration starts from a finite state, and
    // a stage state's y[3..5] is that state plus h * (coefficients of |.| <= 8) * k[3..5],
    // which the clamp bounds by 10 -- finite.
    const int plain = (int)(fabs(d[3]) <= 10.0) & (int)(fabs(d[4]) <= 10.0) &
                      (int)(fabs(d[5]) <= 10.0);
    if (plain) return;
    repair_clamp<!HUGE>(d);
}

// Where the loop-top state recovery (raytracer.c:543-548) can only ever act on the first
// iteration, it runs once, at refill (k_trace), and the hot loop drops its 6 VALU per
// iteration. That holds for RK4 and RKF45 without the far-field branch: every acceleration
// the loop feeds back is a plain |d| <= 10 value or comes out of the literal repair and clamps
// (zero on the Kerr branch), so from a finite state a step adds at most h * 10 * (sum of
// |coefficients| <= 18) to state[3..5] -- a finite double plus that rounds to a finite double
// -- and h times stage values of state[3..5] (bounded by the initial velocities, |v| < 2^512
// for any finite set-up, plus 18 per step) to state[0..2], which cannot reach 2^1024 within
// 2^31 steps. For the same reason RKF45's non-finite-k1 reject (math_util.c:318-333) can
// never fire there.
// The far-field branch's acceleration y5 * 2M / y0^2 is unclamped, but it only runs where
// y0 > 15 rs, so its factor is below C = 2M / (15 rs)^2: per step the velocities grow by at
// most a factor 1 + 2 h W C (plus 20 h W), W the step's largest weight sum. The host proves
// from the scene (far_bounded, scene.c) that a state starting within 2^40 stays below 2^400
// for max_steps steps; far-field instantiations then drop the checks too, and a ray whose
// initial state exceeds 2^40 -- or every ray of a launch the host could not prove bounded --
// is handed to the HUGE redo pass (k_trace's refill), which keeps both checks every iteration.
template <int METHOD, bool FAR, bool HUGE>
constexpr bool repair_at_refill() {
    return (METHOD == INTEGRATOR_RK4 || METHOD == INTEGRATOR_RKF45) && !HUGE;
}

// On the Kerr branch without the far-field one (a != 0, FAR = false) every stage's
// accelerations d[3..5] are the literal 0 (raytracer.c:131-138), so a stage value or update of
// components 3..5 is y + h * (sum of b * 0) = y exactly for the finite state and finite h the
// loop has (only a zero's sign can differ: -0 + +0 = +0). Those components are carried
// unchanged instead of computed (C5: 3 of the 6 components of every RKF45 combination).
template <bool SPIN0, bool FAR>
constexpr bool zero_accel() {
    return !SPIN0 && !FAR;
}

// There, moreover, the stage derivatives of components 0..2 are state[3..5] -- constant over a
// ray's life where the recovery runs once, at refill -- in every stage of every iteration, so
// the weighted stage sums of the step's final combination are per-ray constants: formed once at
// refill (zero_sums, the same expressions on the same values, so bit-identical), and each
// iteration's update of components 0..2 is y + h * sum. RKF45 (C5, two 6-term sums per
// component): +7.5% same-box; RK4 (C4, one 4-term sum, already shared by the iterations of a
// trip) loses 1.5%, so it keeps the inline form (profiles/r02_ab_v24.txt).
template <int METHOD, bool SPIN0, bool FAR, bool HUGE>
constexpr bool hoist_sums() {
    return METHOD == INTEGRATOR_RKF45 && zero_accel<SPIN0, FAR>() &&
           repair_at_refill<METHOD, FAR, HUGE>();
}

// On the same zero-acceleration paths state[2] (theta of the position) advances by a per-ray
// constant times h -- h * (the step's weighted sum of the constant state[5]) -- so within a
// step-size regime the angle turns by the same nominal increment delta every iteration. Its
// sin and cos then follow by a fixed rotation: sin(delta) and cos(delta) - 1 are formed once
// per regime (when h changes, at most three times per ray), and each iteration is the two
// FMA pairs of the shift alone instead of forming delta's polynomials again. The rotation
// tracks the nominal angle, which differs from the rounded state by the states' rounding
// (<= 1 ulp of theta per iteration); the per-iteration shift it replaces carries its own
// rounding the same way.
template <int METHOD, bool SPIN0, bool FAR, bool HUGE>
constexpr bool rotation_trig() {
    return zero_accel<SPIN0, FAR>() && repair_at_refill<METHOD, FAR, HUGE>() &&
           (METHOD == INTEGRATOR_RK4 || METHOD == INTEGRATOR_RKF45);
}

// The step's stage sums (math_util.c:162-207, 367-391), one expression each so that the
// hoisted and the inline forms compile to the same operations.
__device__ __forceinline__ double rk4_acc(double acc, double k) { return acc + 2.0 * k; }
constexpr double kC1 = 25.0 / 216.0, kC3 = 1408.0 / 2565.0, kC4 = 2197.0 / 4104.0,
                 kC5 = -1.0 / 5.0;
constexpr double kD1 = 16.0 / 135.0, kD3 = 6656.0 / 12825.0, kD4 = 28561.0 / 56430.0,
                 kD5 = -9.0 / 50.0, kD6 = 2.0 / 55.0;
__device__ __forceinline__ double rkf45_sum4(double k1, double k3, double k4, double k5) {
    return kC1 * k1 + kC3 * k3 + kC4 * k4 + kC5 * k5;
}
__device__ __forceinline__ double rkf45_sum5(double k1, double k3, double k4, double k5,
                                             double k6) {
    return kD1 * k1 + kD3 * k3 + kD4 * k4 + kD5 * k5 + kD6 * k6;
}

// One reciprocal for two a = 0 stages. x = rc sin theta of a stage needs
// only the position part (components 0, 1) of its state. In RK4 stage 2's is y + h/2 y[3..4],
// known before any acceleration, so x1 and x2 both exist at the top of the iteration; stage 4's
// is y + h (y[3..4] + h/2 k2[3..4]) -- stage 3's velocities, which need stage 2's accelerations
// and nothing of stage 3 -- so x3 and x4 both exist once stage 2 is done. Pairs (1,2) and (3,4):
// w = -2 / (x_a x_b) gives -2 / x_a = x_b w and -2 / x_b = x_a w, one v_rcp_f64 and its
// refinement (7 issue slots) less for three products -- two reciprocals per iteration instead
// of four, no loop-carried register added. Against the single form's
// yr = st RN(1 / RN(rc st)) a member's yr = st RN(x_b RN(1 / RN(x_a x_b))) carries one rounding
// more (x_b's own rounding cancels): five roundings, <= 6 ulp of 1 / rc with the reciprocal's
// own taken as <= 1 ulp (measured worst: profiles/stagepairs/test_figures.txt).
// A member of the far-field branch has no reciprocal to share: it contributes x = 1.
// ok: BOTH members' operands in range (|sin theta| >= 0.01, and rc < 1e150 where that is
// tested): then P = x_a x_b lies in [(0.015 rs)^2, 1e300], normal, and so is w. A member whose
// sin theta is 0, subnormal or NaN -- which would poison or coarsen the shared w -- fails it FOR
// BOTH, and both stages take the literal form with their own reciprocals (accel_fast): a stage
// never uses a quotient derived from an out-of-range partner. (An Inf, which no sine is, passes
// the test and turns both members' quotients into NaN, which fail the plain-value test.)
struct StageOps {
    double st, ct, rc, x;  // sin, cos of the stage's theta, its clamped r, x = rc * st (far: 1)
    bool ok;
};
template <bool HUGE>
__device__ __forceinline__ void stage_x(StageOps& o) {  // x and the range test from st, rc
    o.x = o.rc * o.st;
    o.ok = (!HUGE ? true : o.rc < 1.0e150) & (fabs(o.st) >= 0.01);
}
// NC: 0 shifts from tr with shift_or_eval; 1, 2: tr is a chained anchor (shift_chain<NC>)
template <bool FAR, bool HUGE, int NC = 0>
__device__ __forceinline__ void stage_ops(double y0, double y1, bool far, const Scene& sc,
                                          Counters& n, const Trig1& tr, StageOps& o) {
    if constexpr (NC != 0)
        shift_chain<NC>(tr.a, tr.s, tr.c, y1, o.st, o.ct, HUGE ? nullptr : &n);
    else
        shift_or_eval(tr.a, tr.s, tr.c, y1, o.st, o.ct, HUGE ? nullptr : &n);
    o.rc = max_raw(y0, sc.rs_x1_5);
    stage_x<HUGE>(o);
    if (FAR && far) {
        o.x = 1.0;
        o.ok = true;
    }
}
// wa = -2 / a.x, wb = -2 / b.x from one reciprocal; false: a member is out of range (above)
__device__ __forceinline__ bool pair_rcp(const StageOps& a, const StageOps& b, double& wa,
                                         double& wb) {
    const double w = rcp_nr_m2(a.x * b.x);
    wa = b.x * w;
    wb = a.x * w;
    return a.ok & b.ok;
}
// rhs for a stage whose operands and reciprocal are given (stage_ops, pair_rcp)
template <bool FAR, bool HUGE>
__device__ __forceinline__ void rhs_given(const double (&y)[6], double (&d)[6], const Scene& sc,
                                          bool far, Counters& n, const StageOps& o, double w2,
                                          bool ok) {
    d[0] = y[3];
    d[1] = y[4];
    d[2] = y[5];
    if (FAR && far) {  // weak-field branch, as in rhs
        d[3] = 0.0;
        d[4] = 0.0;
        d[5] = y[5] * (sc.two_m / (y[0] * y[0]));
        n.far_++;
        return;
    }
    if ((FAR && HUGE) || BHRT_COUNT_STAGES) n.full++;
    accel_fast<HUGE, true>(y, d, sc, o.st, o.ct, o.rc, w2, ok);
}

// rk4_integrate (math_util.c:162-207) on the six live components; the running sum
// ((k1 + 2k2) + 2k3) + k4 is the reference's left-to-right evaluation order. Two forms: the
// a = 0 step (SPIN0) with its paired reciprocals and chained shifts, and the generic step.
template <bool SPIN0, bool FAR, bool HUGE, bool HS = false>
__device__ __forceinline__ void rk4_step(double (&y)[6], double h, double h6, const Scene& sc,
                                         bool far_ok, Counters& n, Trig1& tr,
                                         const double* zs = nullptr) {
    double k[6], acc[6], yt[6];
    const double hh = 0.5 * h;
    if constexpr (SPIN0) {
        // stages 1, 2 on one reciprocal and stages 3, 4 on another (pair_rcp). The position
        // parts formed ahead are the very expressions the stage-state loops would form
        // (k[0..1] of a stage are its state's [3..4]).
        // Chained anchors (shift_chain): stage 3's theta from stage 2's (an), and t4, stage 4's
        // theta with its sin, cos, handed back in tr for the caller's advance of state[1] (a
        // stage 2 or 4 on the far-field branch takes no sin, cos: the anchor then stays tr)
        const double y20 = y[0] + hh * y[3], y21 = y[1] + hh * y[4];
        const bool far1 = FAR && far_ok && y[0] > sc.rs_x15;
        const bool far2 = FAR && far_ok && y20 > sc.rs_x15;
        StageOps o1, o2, o3, o4;
        double w1 = 0.0, w2 = 0.0, w3 = 0.0, w4 = 0.0;
        bool ok = false;
        Trig1 an = tr, t4 = tr;
        if (!FAR || !(far1 & far2)) {
            o1.st = tr.s;  // carried from the previous iteration (ray_iterate)
            o1.ct = tr.c;
            o1.rc = max_raw(y[0], sc.rs_x1_5);
            stage_x<HUGE>(o1);
            if (FAR && far1) {
                o1.x = 1.0;
                o1.ok = true;
            }
            stage_ops<FAR, HUGE>(y20, y21, far2, sc, n, tr, o2);
            an = Trig1{y21, o2.st, o2.ct};
            ok = pair_rcp(o1, o2, w1, w2);
        }
        rhs_given<FAR, HUGE>(y, k, sc, far1, n, o1, w1, ok);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc[i] = k[i];
            yt[i] = i == 0 ? y20 : i == 1 ? y21 : y[i] + hh * k[i];
        }
        rhs_given<FAR, HUGE>(yt, k, sc, far2, n, o2, w2, ok);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc[i] = rk4_acc(acc[i], k[i]);
            yt[i] = y[i] + hh * k[i];
        }
        const double y40 = y[0] + h * yt[3], y41 = y[1] + h * yt[4];
        const bool far3 = FAR && far_ok && yt[0] > sc.rs_x15;
        const bool far4 = FAR && far_ok && y40 > sc.rs_x15;
        ok = false;
        if (!FAR || !(far3 & far4)) {
            stage_ops<FAR, HUGE, 2>(yt[0], yt[1], far3, sc, n, an, o3);
            stage_ops<FAR, HUGE>(y40, y41, far4, sc, n, tr, o4);
            t4 = Trig1{y41, o4.st, o4.ct};
            ok = pair_rcp(o3, o4, w3, w4);
        }
        rhs_given<FAR, HUGE>(yt, k, sc, far3, n, o3, w3, ok);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc[i] = rk4_acc(acc[i], k[i]);
            yt[i] = i == 0 ? y40 : i == 1 ? y41 : y[i] + h * k[i];
        }
        rhs_given<FAR, HUGE>(yt, k, sc, far4, n, o4, w4, ok);
#pragma unroll
        for (int i = 0; i < 6; i++) y[i] = __builtin_fma(h6, acc[i] + k[i], y[i]);
        tr = t4;
    } else {
        // Z: components 3..5 carried unchanged (zero_accel); HS: zs holds the hoisted stage sums
        // of components 0..2 (hoist_sums)
        constexpr bool Z = zero_accel<SPIN0, FAR>();
        rhs<SPIN0, FAR, HUGE>(y, k, sc, far_ok, n, tr, true);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc[i] = k[i];
            yt[i] = (Z && i >= 3) ? y[i] : y[i] + hh * k[i];
        }
        rhs<SPIN0, FAR, HUGE>(yt, k, sc, far_ok, n, tr, false);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc[i] = rk4_acc(acc[i], k[i]);
            yt[i] = (Z && i >= 3) ? y[i] : y[i] + hh * k[i];
        }
        rhs<SPIN0, FAR, HUGE>(yt, k, sc, far_ok, n, tr, false);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            acc[i] = rk4_acc(acc[i], k[i]);
            yt[i] = (Z && i >= 3) ? y[i] : y[i] + h * k[i];
        }
        rhs<SPIN0, FAR, HUGE>(yt, k, sc, far_ok, n, tr, false);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            // h * (...) / 6 as (h * RN(1/6)) * (...), h6 = h * RN(1/6) (the caller's): the
            // increment differs by <= 1 ulp of itself, which is ~h*|k| / |y| ulp of the state
            if (HS && i < 3)
                y[i] = __builtin_fma(h6, zs[i], y[i]);
            else if (!(Z && i >= 3))
                y[i] = __builtin_fma(h6, acc[i] + k[i], y[i]);
        }
    }
}

// RKF45's accept test (math_util.c:367-391, 402-434): accept iff
// RN(max_i RN(err_i / scale_i) / tol) <= 1, scale_i >= 1e-10. For a positive normal (finite)
// tol the outer test is exactly max_error <= tol: x <= t gives x / t <= 1; x > t means
// x >= t + ulp(t), so x / t >= 1 + ulp(t) / t > 1 + 2^-53, the rounding midpoint above 1
// (x = Inf: Inf / t = Inf > 1, also a reject). That is, every component's RN(err / scale) <=
// tol. FAST (where the state is provably bounded, repair_at_refill: |scale| < 2^600) with tol
// in [2^-900, 2^300] decides a component without a division: err <= RN(tol (1 - 2^-40) scale)
// passes, err > RN(tol (1 + 2^-40) scale) rejects, and only an err inside that band (per lane,
// rare) takes the IEEE quotient (v24; v17-v23 formed q = err * rcp(scale) and compared it with
// the same band, 4 more VALU per component; v25 first tries the one-sided test alone, which
// accepts when every component passes it: one product and one compare per component). Otherwise, and for a tol that is <= 0,
// subnormal, Inf or NaN, the literal final quotient decides (wave-uniform branch on tol):
// tol = Inf with max_error = Inf is Inf / Inf = NaN, a reject, where max_error <= tol would
// accept. bhrt_check_rkf45_accept runs both forms on given operands
// (tests/test_gpu_parity.py::test_rkf45_accept_band).
template <bool FAST, int NC = 6>
__device__ __forceinline__ bool rkf45_accept(const double (&err)[6], const double (&scale)[6],
                                             double tol) {
    const bool tol_normal = tol >= 2.2250738585072014e-308 && tol <= 1.79769313486231570815e+308;
    if (FAST && tol >= 0x1p-900 && tol <= 0x1p300) {
        // tol * scale is a normal product here (scale in [1e-10, 2^600]), so RN(lo * scale) and
        // RN(hi * scale) are within 2^-53 of the exact products
        const double lo = tol * (1.0 - 0x1p-40), hi = tol * (1.0 + 0x1p-40);
        // every component clearly inside tol (the usual case): accept with one product and
        // one compare per component; otherwise the two-sided test below
        bool all_pass = true;
#pragma unroll
        for (int i = 0; i < NC; i++) all_pass &= err[i] <= lo * scale[i];
        if (__builtin_expect(all_pass, 1)) return true;
        double near_max = 0.0;
        bool over = false;
#pragma unroll
        for (int i = 0; i < NC; i++) {  // components NC.. have err = 0 (zero_accel)
            // err <= RN(lo s): err / s < tol (1 - 2^-41), so RN(err / s) <= tol;
            // err > RN(hi s): err / s > tol (1 + 2^-41) > tol + ulp(tol) / 2, a reject
            const bool pass = err[i] <= lo * scale[i];
            const bool fail = err[i] > hi * scale[i];
            over |= fail;
            if (__builtin_expect(!pass && !fail, 0)) near_max = fmax(near_max, err[i] / scale[i]);
        }
        return !over && near_max <= tol;
    }
    double max_error = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) max_error = fmax(max_error, err[i] / scale[i]);
    return tol_normal ? max_error <= tol : max_error / tol <= 1.0;
}

// Attempts that cannot be rejected (ACC; round 6). Where the stage sums are hoisted (hoist_sums:
// the zero-acceleration paths, C5) every stage derivative of components 0..2 is the ray's
// constant v = state[3..5], so s4 = rkf45_sum4(v, v, v, v) and s5 = rkf45_sum5(v, ..., v) are v
// times weight sums that are exactly 1 in real arithmetic, each within E <= 10u |v| of v (u =
// 2^-53: <= 5 products and sums, partial sums below 1.5 |v|, the weights' own rounding). The
// attempt's a = y5 = RN(y + h s5), b = y4 = RN(y + h s4) and err = RN(|a - b|) then satisfy
//   |a - b| <= |h| |s5 - s4| + u (|a| + |b|)  and  |b| <= |a| + |a - b|,
// so |a - b| <= (|h| |s5 - s4| + 2u |a|) / (1 - u). And scale = max(|y|, |a|, 1e-10) >= |h v| / 2.1
// (if |y| < |h v| / 2, then |a| >= |h v| (1 - E) - |y| - u |a|). Hence err / scale <= 2.1 * 2E
// + 2u (1 + 3u) < 50u < 6e-15 for every component (v = 0: s4 = s5 = 0 and err = 0 exactly;
// tiny v: the absolute rounding is below 2^-1074 against scale >= 1e-10), whatever the state:
// every attempt passes the accept test -- RN(max err / scale) / tol <= 1 -- for any
// tol >= 2^-30 (the host's condition, scene.c bhrt_fill_scene: accept_all, with finite step
// sizes and tol <= 2^300). The attempt is then y <- y5 alone: no y4, error, scale or test, and no
// fixed point (C5: ~20 of ~87 VALU per attempt). The state is finite there (repair_at_refill),
// so y + h s5 is too. The redo pass (HUGE) keeps the literal test.
template <bool SPIN0, bool FAR, bool HUGE>
constexpr bool accept_all_ok() {
    return zero_accel<SPIN0, FAR>() && repair_at_refill<INTEGRATOR_RKF45, FAR, HUGE>();
}

// rkf45_integrate (math_util.c:212-457), n = 6. Returns true on accept (y <- y5).
template <bool SPIN0, bool FAR, bool HUGE, bool HS = false, bool ACC = false>
__device__ __forceinline__ bool rkf45_attempt(double (&y)[6], double h, const Scene& sc,
                                              bool far_ok, Counters& n, Trig1& tr,
                                              const double* zs = nullptr) {
    static_assert(!ACC || (HS && accept_all_ok<SPIN0, FAR, HUGE>()), "ACC: hoisted sums only");
    constexpr double b21 = 1.0 / 4.0;
    constexpr double b31 = 3.0 / 32.0, b32 = 9.0 / 32.0;
    constexpr double b41 = 1932.0 / 2197.0, b42 = -7200.0 / 2197.0, b43 = 7296.0 / 2197.0;
    constexpr double b51 = 439.0 / 216.0, b52 = -8.0, b53 = 3680.0 / 513.0,
                     b54 = -845.0 / 4104.0;
    constexpr double b61 = -8.0 / 27.0, b62 = 2.0, b63 = -3544.0 / 2565.0,
                     b64 = 1859.0 / 4104.0, b65 = -11.0 / 40.0;
    double k1[6], k2[6], k3[6], k4[6], k5[6], k6[6], yt[6];
    rhs<SPIN0, FAR, HUGE>(y, k1, sc, far_ok, n, tr, true);
    if (!repair_at_refill<INTEGRATOR_RKF45, FAR, HUGE>()) {
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 6; i++) bad |= !isfinite(k1[i]);  // :318-333
        if (bad) return false;
    }
    const double hb21 = h * b21;
    constexpr bool Z = zero_accel<SPIN0, FAR>();  // components 3..5 stay y (zero_accel)
#pragma unroll
    for (int i = 0; i < 6; i++) yt[i] = (Z && i >= 3) ? y[i] : y[i] + hb21 * k1[i];
    rhs<SPIN0, FAR, HUGE>(yt, k2, sc, far_ok, n, tr, false);
#pragma unroll
    for (int i = 0; i < 6; i++)
        yt[i] = (Z && i >= 3) ? y[i] : y[i] + h * (b31 * k1[i] + b32 * k2[i]);
    rhs<SPIN0, FAR, HUGE>(yt, k3, sc, far_ok, n, tr, false);
#pragma unroll
    for (int i = 0; i < 6; i++)
        yt[i] = (Z && i >= 3) ? y[i] : y[i] + h * (b41 * k1[i] + b42 * k2[i] + b43 * k3[i]);
    rhs<SPIN0, FAR, HUGE>(yt, k4, sc, far_ok, n, tr, false);
#pragma unroll
    for (int i = 0; i < 6; i++)
        yt[i] = (Z && i >= 3) ? y[i]
                              : y[i] + h * (b51 * k1[i] + b52 * k2[i] + b53 * k3[i] + b54 * k4[i]);
    rhs<SPIN0, FAR, HUGE>(yt, k5, sc, far_ok, n, tr, false);
#pragma unroll
    for (int i = 0; i < 6; i++)
        yt[i] = (Z && i >= 3) ? y[i]
                              : y[i] + h * (b61 * k1[i] + b62 * k2[i] + b63 * k3[i] +
                                            b64 * k4[i] + b65 * k5[i]);
    rhs<SPIN0, FAR, HUGE>(yt, k6, sc, far_ok, n, tr, false);
    if constexpr (ACC) {  // never rejected (above): y <- y5, the same expression as below
#pragma unroll
        for (int i = 0; i < 3; i++) y[i] = y[i] + h * zs[3 + i];
        return true;
    }
    double y5[6];
    // :367-391 and :402-434 (rkf45_accept)
    constexpr bool FAST_NORM = repair_at_refill<INTEGRATOR_RKF45, FAR, HUGE>();
    double err[6], scale[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        if (Z && i >= 3) {  // y4 = y5 = y: error 0
            y5[i] = y[i];
            scale[i] = fmax(fabs(y[i]), kEps);
            err[i] = 0.0;
            continue;
        }
        const double s4 = HS ? zs[i] : rkf45_sum4(k1[i], k3[i], k4[i], k5[i]);
        const double s5 = HS ? zs[3 + i] : rkf45_sum5(k1[i], k3[i], k4[i], k5[i], k6[i]);
        const double y4 = y[i] + h * s4;
        y5[i] = y[i] + h * s5;
        if (FAST_NORM) {
            // the state is finite and bounded here (repair_at_refill), so y and y5 are not NaN
            // and fmax / the kEps floor are plain maxima: two v_max_f64 instead of five VALU
            scale[i] = max_raw(max_abs_raw(y[i], y5[i]), kEps);
        } else {
            scale[i] = fmax(fabs(y[i]), fabs(y5[i]));
            if (scale[i] < kEps) scale[i] = kEps;
        }
        err[i] = fabs(y5[i] - y4);
    }
    // a zero error passes the fast form's per-component test for any positive normal tol, so
    // the fast form looks at the live components only; the literal form keeps all six (its
    // fmax chain would turn an earlier NaN into the 0 of a later component, as the
    // reference's does)
    const bool accept = rkf45_accept<FAST_NORM, (Z && FAST_NORM) ? 3 : 6>(err, scale, sc.tol);
    if (accept) {
#pragma unroll
        for (int i = 0; i < 6; i++) y[i] = y5[i];
        return true;
    }
    return false;
}

// spherical_to_cartesian (spacetime.c:229-237) from carried sin/cos
__device__ __forceinline__ void sph2cart_t(double r, double st, double ct, double sp, double cp,
                                           double& x, double& y, double& z) {
    x = r * st * cp;
    y = r * st * sp;
    z = r * ct;
}

// sin, cos of x from those of a, the same component one iteration earlier.
// Per ray only (never dependent on which wave runs the ray), so results stay reproducible.
__device__ __forceinline__ void trig_advance(double a, double x, double& s, double& c,
                                             Counters* hc) {
    double s1, c1;
    shift_or_eval(a, s, c, x, s1, c1, hc);
    s = s1;
    c = c1;
}

// sqrt as the compiler's f64 expansion computes it (v_rsq_f64, Goldschmidt refinement, two
// residual corrections) without its denormal scaling and Inf/0 class fix-up, which only
// x < 2^-767 needs -- those lanes take the library sqrt.
__device__ __forceinline__ double sqrt_nr(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double s = x * y, hy = y * 0.5;
    const double r = __builtin_fma(-hy, s, 0.5);
    s = __builtin_fma(s, r, s);
    hy = __builtin_fma(hy, r, hy);
    double e = __builtin_fma(-s, s, x);
    s = __builtin_fma(e, hy, s);
    e = __builtin_fma(-s, s, x);
    s = __builtin_fma(e, hy, s);
    // one rare branch (not an if / else pair of exec-mask regions around both forms)
    if (__builtin_expect(!(x >= 0x1p-767), 0)) s = sqrt(x);
    return s;
}

// sqrt_nr with ONE residual correction: v_rsq_f64 is good to ~2^-24, the
// Goldschmidt step squares that, and one s += (x - s^2) * hy leaves an error far below the final
// rounding, so only an argument whose root lies next to a rounding midpoint can come out one
// ulp off: <= 1 ulp, measured 0 ulp from sqrt on 1e5 arguments over [2^-700, 2^600]
// (tests/test_gpu_loop_tail.py). Two VALU fewer, and two links off the iteration's dependent
// chain.
__device__ __forceinline__ double sqrt_nr1(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double s = x * y, hy = y * 0.5;
    const double r = __builtin_fma(-hy, s, 0.5);
    s = __builtin_fma(s, r, s);
    hy = __builtin_fma(hy, r, hy);
    const double e = __builtin_fma(-s, s, x);
    s = __builtin_fma(e, hy, s);
    if (__builtin_expect(!(x >= 0x1p-767), 0)) s = sqrt(x);
    return s;
}

__device__ __forceinline__ double len3(double x, double y, double z) {
    return sqrt((x * x + y * y) + z * z);  // vector3D_length (math_util.c:85-113)
}
// the per-iteration path length |p - p_prev| of the hot loop: it only feeds the running
// distance (a sum of up to max_steps of them, compared with max_dist).
// sqrt_nr1(+Inf) is NaN (rsq gives 0, and Inf * 0), where vector3D_length's sqrt is +Inf and the
// ray ends as MAX_DISTANCE: a segment from an infinite origin, or one whose squares overflow
// (longer than 1.3e154). WIDE (the general instantiation: k_path, k_paths, the HUGE redo) keeps
// the reference's value there; the hot instantiations never see such a segment behind a finite
// origin (their state is bounded, repair_at_refill).
template <bool WIDE>
__device__ __forceinline__ double seg_len(double x, double y, double z) {
    const double q = (x * x + y * y) + z * z;
    const double s = sqrt_nr1(q);
    if (WIDE) return q == __builtin_inf() ? q : s;
    return s;
}

struct Ray_ {
    double y[6];        // (t, r, theta, phi, tdot, rdot)
    double y6, y7;      // (thetadot, phidot): constants, see header
    double dx, dy, dz;  // Ray.direction as given (disk test)
    double px, py, pz;  // current Cartesian position; the disk hit point once T_DISK
    double dist;
    double s1, c1, s2, c2, s3, c3;  // sin, cos of y[1], y[2], y[3] (carried)
    double zs[6];       // per-ray stage sums of components 0..2 (hoist_sums)
    double cd_sd, cd_cm1;        // rotation_trig: sin(delta) and cos(delta) - 1 of the
                                 // increment at the step size h (set with it, hcache)
    double h, h_lo, h_hi;        // hcache: the step size and the r interval it holds on
    double h6;                   // h * RN(1/6), kept with h where h6cache() (RK4's final update)
    int k;              // iterations executed
    bool far_ok;        // use_analytic_approx && impact_parameter > 0
};

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

__device__ __forceinline__ void trig_anchor(Ray_& R, Counters* hc = nullptr) {
    bhrt_sincos(R.y[1], &R.s1, &R.c1, hc);
    bhrt_sincos(R.y[2], &R.s2, &R.c2, hc);
    bhrt_sincos(R.y[3], &R.s3, &R.c3, hc);
}

// Trig-free part of integrate_photon_path's set-up (raytracer.c:355-466): the initial
// velocities, dt/dlambda from the null condition, E, L, b. s_* are products of the origin's
// sin/cos, g_* the metric at the origin.
__device__ __forceinline__ void init_velocity(Ray_& R, double nx, double ny, double nz,
                                              double r, double st_cp, double st_sp, double ct,
                                              double ct_cp, double ct_sp, double st,
                                              double neg_sp, double cp, double r_st,
                                              bool st_tiny, double g_tt, double g_rr,
                                              double g_hh, bool use_approx) {
    const double vr = st_cp * nx + st_sp * ny + ct * nz;            // :389-391
    const double vth = (ct_cp * nx + ct_sp * ny - st * nz) / r;     // :394-396
    double vph = (neg_sp * nx + cp * ny) / r_st;                    // :399
    if (st_tiny) vph = 0.0;                                         // :402-405
    double dt2 = -(g_rr * vr * vr + g_hh * vth * vth + g_hh * vph * vph) / g_tt;  // :416-418
    if (dt2 < 0.0) dt2 = 0.0;
    const double vt = sqrt(dt2);
    const double b = fabs((g_hh * vph) / (-g_tt * vt));  // |L / E| (:437-448)
    R.far_ok = use_approx && (b > 0.0);
    R.y[4] = vt;
    R.y[5] = vr;
    R.y6 = isfinite(vth) ? vth : 0.0;  // recovery of :543-548 for the constant components
    R.y7 = isfinite(vph) ? vph : 0.0;
}

__device__ __forceinline__ void normalize3(double x, double y, double z, double& nx, double& ny,
                                           double& nz) {
    const double l = len3(x, y, z);  // vector3D_normalize (math_util.c:115-122)
    if (l < kEps) {
        nx = ny = nz = 0.0;
    } else {
        const double inv = 1.0 / l;
        nx = x * inv;
        ny = y * inv;
        nz = z * inv;
    }
}

// Full per-ray set-up for an arbitrary origin (ray arrays, single-ray path kernel).
__device__ __forceinline__ void ray_init_general(Ray_& R, double t0, double ox, double oy,
                                                 double oz, double dx, double dy, double dz,
                                                 const Scene& sc) {
    R.dx = dx;
    R.dy = dy;
    R.dz = dz;
    double nx, ny, nz;
    normalize3(dx, dy, dz, nx, ny, nz);
    const double r = sqrt(ox * ox + oy * oy + oz * oz);  // cartesian_to_spherical
    const double th = (r > kEps) ? acos(oz / r) : 0.0;
    double ph = atan2(oy, ox);
    if (ph < 0.0) ph += kTwoPi;
    double st, ct, sp, cp;
    sincos(th, &st, &ct);
    sincos(ph, &sp, &cp);
    const double rm = (r <= sc.rs_eps) ? sc.rs_eps : r;  // calculate_schwarzschild_metric
    const double g_tt = -(1.0 - sc.rs / rm);
    const double g_rr = 1.0 / (1.0 - sc.rs / rm);
    const double g_hh = rm * rm;  // g_thth = g_phph (sin^2(pi/2) == 1)
    init_velocity(R, nx, ny, nz, r, st * cp, st * sp, ct, ct * cp, ct * sp, st, -sp, cp, r * st,
                  fabs(st) < kEps, g_tt, g_rr, g_hh, r > sc.rs_x15);
    R.y[0] = t0;
    R.y[1] = r;
    R.y[2] = th;
    R.y[3] = ph;
    R.px = r * st * cp;  // spherical_to_cartesian of the initial state (:498-501)
    R.py = r * st * sp;
    R.pz = r * ct;
    R.dist = 0.0;
    R.k = 0;
}

// floor(a / d) for 0 <= a < 2^31, d >= 1, from inv = RN(1 / d): RN(a * inv) is within 2^-52
// relative of a / d, so its truncation is the quotient or one below it (never above: a / d
// ends at least 1 / d short of the next integer, and d (q + 1) < 2^52), and one test fixes it
// -- a few VALU instead of the ~30 of a 32-bit integer division
__device__ __forceinline__ int div_floor(int a, int d, double inv) {
    int q = (int)((double)a * inv);
    if ((unsigned)(q + 1) * (unsigned)d <= (unsigned)a) q++;
    return q;
}

// calculate_ray_direction (raytracer.c:1013-1038) for pixel-centre ray i of the shard
__device__ __forceinline__ void camera_dir(const bhrt_camera_k& cm, int i, double& dx,
                                           double& dy, double& dz) {
    const int W = cm.width;
    const int j = div_floor(i, W, cm.inv_width), px = i - j * W;
    int py = j;
    if (cm.rows.num_shards > 1) {
        const int B = cm.rows.row_block;
        const int jb = div_floor(j, B, cm.inv_block);
        py = (jb * cm.rows.num_shards + cm.rows.shard) * B + (j - jb * B);
    }
    const double ndcx = (2.0 * ((px + cm.off_x) / W) - 1.0) * cm.plane_w;
    const double ndcy = (1.0 - 2.0 * ((py + cm.off_y) / cm.height)) * cm.plane_h;
    double vx = cm.fwd[0], vy = cm.fwd[1], vz = cm.fwd[2];
    vx = vx + cm.right[0] * ndcx;
    vy = vy + cm.right[1] * ndcx;
    vz = vz + cm.right[2] * ndcx;
    vx = vx + cm.up[0] * ndcy;
    vy = vy + cm.up[1] * ndcy;
    vz = vz + cm.up[2] * ndcy;
    normalize3(vx, vy, vz, dx, dy, dz);
}

// Camera ray set-up: the origin is shared, so only the direction-dependent part runs here.
__device__ __forceinline__ void ray_init_camera(Ray_& R, const bhrt_camera_k& cm, int i) {
    camera_dir(cm, i, R.dx, R.dy, R.dz);
    double nx, ny, nz;
    normalize3(R.dx, R.dy, R.dz, nx, ny, nz);  // integrate_photon_path normalises again
    init_velocity(R, nx, ny, nz, cm.r0, cm.st_cp, cm.st_sp, cm.ct, cm.ct_cp, cm.ct_sp, cm.st,
                  cm.neg_sp, cm.cp, cm.r_st, cm.st_tiny != 0, cm.g_tt, cm.g_rr, cm.g_hh,
                  cm.use_approx != 0);
    R.y[0] = 0.0;
    R.y[1] = cm.r0;
    R.y[2] = cm.th0;
    R.y[3] = cm.ph0;
    R.px = cm.p0[0];
    R.py = cm.p0[1];
    R.pz = cm.p0[2];
    R.dist = 0.0;
    R.k = 0;
}

// A ray of an array whose rays all start at the launch's shared origin (kp.rays_shared): the
// origin part of the set-up is the host's (cm, as for a camera frame); the direction is the
// array's, kept as given for the disk test (Ray.direction) and normalised for the velocities,
// as ray_init_general does.
__device__ __forceinline__ void ray_init_shared(Ray_& R, const bhrt_camera_k& cm,
                                                const double* dirs, int stride, int i) {
    const double* d = dirs + (size_t)i * stride;
    R.dx = d[0];
    R.dy = d[1];
    R.dz = d[2];
    double nx, ny, nz;
    normalize3(R.dx, R.dy, R.dz, nx, ny, nz);
    init_velocity(R, nx, ny, nz, cm.r0, cm.st_cp, cm.st_sp, cm.ct, cm.ct_cp, cm.ct_sp, cm.st,
                  cm.neg_sp, cm.cp, cm.r_st, cm.st_tiny != 0, cm.g_tt, cm.g_rr, cm.g_hh,
                  cm.use_approx != 0);
    R.y[0] = 0.0;
    R.y[1] = cm.r0;
    R.y[2] = cm.th0;
    R.y[3] = cm.ph0;
    R.px = cm.p0[0];
    R.py = cm.p0[1];
    R.pz = cm.p0[2];
    R.dist = 0.0;
    R.k = 0;
}

// check_disk_intersection (raytracer.c:159-196), plane "normal" = previous path point n,
// straight-line. The radial test compares s = qx^2 + qy^2 against the host's thresholds instead
// of taking sqrt(s) (scene.c sqrt_lower/upper_bound).
// Every iteration only SCREENS its segment, without a quotient (disk_cand):
// with t = num / den, den * q = p den + d num, so S = (px den + dx num)^2 + (py den + dy num)^2
// = s den^2 is compared with the thresholds times den^2, and t < 0 is num den < 0. The four
// rejections are ONE mask (a per-test early return became nested exec-mask regions, ~50 SALU
// per iteration). A lane that passes the screen -- about once per hitting ray -- then makes the
// reference's decision literally, in a rare branch (disk_decide): |den| < 1e-10, t by the IEEE
// quotient, t < 0, the point, s against the thresholds. So a hit is always one the literal form
// accepts, and the screen only has to pass every lane the literal form could accept:
//   - |den| >= big (2^100), a NaN or Inf den included, passes unscreened: below it den^2, the
//     scaled thresholds and S stay finite for points and directions below 2^100 and radii
//     below 2^400 (far beyond them an S that overflows to Inf fails the outer comparison
//     unless that threshold is Inf too);
//   - the sign test rejects only den (num + 2^-1000 den) < 0, i.e. t < -2^-1000, where
//     RN(num / den) is a negative normal. A t that is or rounds to -0.0 (num = +-0, or an
//     underflowed quotient), which the reference accepts, is never rejected; nor is a product
//     that underflows to -0;
//   - |den| < 1e-10 is left to the literal form;
//   - S carries two roundings per component where the reference's s carries those of t, d t
//     and p + d t: the screen and the literal form can only disagree for a candidate point
//     within a few ulp of a rim, where the screen may reject a point the reference accepts
//     by that margin (never the other way round).
// A NaN operand fails the screen's comparisons as it fails the reference's. Radii whose
// squares times den^2 would be subnormal (below ~1e-144) are screened at the subnormals'
// precision.
// FAR TESTS FIRST. On a ray that never hits, the candidate point lies far outside the outer rim
// in every iteration (C2, camera B: median |q_xy| 193 against 20), and ONE component against that
// rim already says so: sx^2 > out_sq den^2 for every live lane of 94% of the wave-iterations
// (tools/screen_replay.py). So the fall-through path forms only den, num, d2, sx, sxx = RN(sx sx)
// and the outer threshold T = RN(out_sq d2): a lane with sxx > T and |den| < big is rejected at
// once. The others (a NaN operand and |den| >= big among them: their comparisons fail) go on in
// a rare, exec-masked block that tries RN(sy sy) > T the same way, and only a lane that
// survives both forms sg, S and the inner threshold and takes the one-mask screen above.
// Neither far test rejects a lane that screen passes:
//   - RN(sy sy) >= 0, so sx sx + RN(sy sy) >= sx sx exactly; rounding is monotone, so
//     S = fma(sx, sx, RN(sy sy)) >= RN(sx sx) = sxx, or S is NaN. Either way S <= T is false
//     whenever sxx > T. (sxx is a product of its own, for the test alone: S keeps its FMA.)
//   - likewise S >= RN(sy sy): the FMA rounds the exact sx sx + RN(sy sy) >= RN(sy sy) once;
//   - with |den| < big required, the unscreened pass does not apply.
// So the lanes that reach disk_decide are the same set, and every output the same bits
// (profiles/farscreen/bitexact.txt; tests/test_far_screen_cpu.py checks the implication on
// 1e5 operand sets in exact arithmetic).
__device__ __forceinline__ bool disk_cand(const Ray_& R, double nx, double ny, double nz,
                                          const Scene& sc, double big, double& num,
                                          double& den) {
    den = (R.dx * nx + R.dy * ny) + R.dz * nz;
    num = -((R.px * nx + R.py * ny) + R.pz * nz);
    const double d2 = den * den;
    const double sx = __builtin_fma(R.dx, num, R.px * den);
    const double sxx = sx * sx;  // for the far test alone: S below keeps its own rounding
    const double out = sc.disk_out_sq * d2;
    bool cand = false;
    if (__builtin_expect(!((sxx > out) & (fabs(den) < big)), 0)) {
        // |den| < big again, of a copy the optimiser cannot see through: kept live across the
        // branch, the mask cost the fall-through path a second compare of the same operands
        double dn = den;
        asm volatile("" : "+v"(dn));
        const bool small = fabs(dn) < big;
        const double sy = __builtin_fma(R.dy, num, R.py * den);
        const double syy = sy * sy;
        if (!((syy > out) & small)) {
            const double sg = den * __builtin_fma(0x1p-1000, den, num);
            const double S = __builtin_fma(sx, sx, syy);
            cand = (!(sg < 0.0) & (S >= sc.disk_in_sq * d2) & (S <= out)) | !small;
        }
    }
    return cand;
}

// The reference's decision for a lane that passed the screen, and its candidate point
__device__ __forceinline__ bool disk_decide(const Ray_& R, double num, double den,
                                            const Scene& sc, double& qx, double& qy,
                                            double& qz) {
    const double t = num / den;
    qx = R.px + R.dx * t;
    qy = R.py + R.dy * t;
    qz = R.pz + R.dz * t;
    const double s = qx * qx + qy * qy;
    return !(fabs(den) < kEps) & !(t < 0.0) & (s >= sc.disk_in_sq) & (s <= sc.disk_out_sq);
}

__device__ __forceinline__ bool disk_hit(const Ray_& R, double nx, double ny, double nz,
                                         const Scene& sc, double big, double& qx, double& qy,
                                         double& qz) {
    double num, den;
    return disk_cand(R, nx, ny, nz, sc, big, num, den) &&
           disk_decide(R, num, den, sc, qx, qy, qz);
}

enum Term : int { T_NONE = 0, T_HORIZON, T_DISK, T_MAXDIST, T_MAXSTEPS };

// p_{k-1}, the point a ray's last iteration started from, for the sky lookup at its exit: the
// exit chord is p_k - p_{k-1}, taken there (exit_chord). Only the point is kept in the loop -- a
// copy, no arithmetic -- so that the sky instantiations' iterations are the plain ones' operation
// for operation (a difference formed in the loop would give the compiler other products to
// contract, and a disk hit other bits). Kept beside Ray_, by k_trace's sky instantiations alone: as
// a part of Ray_ it would grow the stack objects of the kernels that hold the ray in memory (the
// redo pass, k_path) whether they have a sky or not.
struct Chord {
    double x, y, z;
};
// RN(p_k - p_{k-1}) per component, no contraction: what the rule's reader forms from two path points
__device__ __forceinline__ void exit_chord(const Chord& prev, double px, double py, double pz,
                                           double& cx, double& cy, double& cz) {
#pragma clang fp contract(off)
    cx = px - prev.x;
    cy = py - prev.y;
    cz = pz - prev.z;
}

struct HSel {  // the four step sizes of the schedule, hoisted out of the kernel argument block
    double far_, r15, r5, r2_5;
    double big;  // 2^100, the disk test's bound on |den| (disk_hit): an SGPR pair set once,
                 // outside the loop (as a literal it was rematerialised by two s_mov in every
                 // iteration)
};

// x unchanged, but opaque to the optimiser: the four step sizes stay four register values
// selected by v_cndmask. Left visible as loads, the select chain over them became ONE load at a
// selected address, and the promoted step-size array an LDS table: a ds_read_b64 and an
// lgkmcnt wait at the head of every iteration's dependency chain.
template <bool V>
__device__ __forceinline__ double opaque(double x) {
    if (V)
        asm volatile("" : "+v"(x));
    else
        asm volatile("" : "+s"(x));
    return x;
}
// V: the step sizes in VGPRs (8 more registers; each select is then one v_cndmask per half
// instead of a v_mov from the SGPR and a v_cndmask): where the loop has registers to spare
template <bool V = false>
__device__ __forceinline__ HSel hsel_of(const Scene& sc) {
    return HSel{opaque<V>(sc.h_far), opaque<V>(sc.h_15), opaque<V>(sc.h_5), opaque<V>(sc.h_2_5),
                opaque<false>(0x1p100)};
}

// :543-548, state NaN/Inf recovery at the top of an iteration. One test of the sum
// (non-finite if any component is, or on overflow); the per-component repair runs only then.
// ANCHOR = false: the caller knows state[1..3] are finite, so their sin/cos stay valid.
template <bool ANCHOR = true>
__device__ __forceinline__ void state_repair(Ray_& R, Counters* hc) {
    if (__builtin_expect(
            !isfinite(((R.y[0] + R.y[1]) + (R.y[2] + R.y[3])) + (R.y[4] + R.y[5])), 0)) {
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (!isfinite(R.y[i])) R.y[i] = (i < 4) ? 1.0 : 0.0;
        if (ANCHOR) trig_anchor(R, hc);
    }
}

// every component of the state within +-bound (NaN fails)
__device__ __forceinline__ bool state_within(const Ray_& R, double bound) {
    const double m = fmax(fmax(fmax(fabs(R.y[0]), fabs(R.y[1])), fmax(fabs(R.y[2]), fabs(R.y[3]))),
                          fmax(fabs(R.y[4]), fabs(R.y[5])));
    return m <= bound;
}

// Where the step size is kept per ray with its r interval (ray_iterate): every RK4 path. C4's
// ~80-VALU iteration spent 9 on the select chain: -3.6% kernel time same-box, bit-identical
// (round 3). C2 measured neutral then; with round 6's wave-uniform trip it is +1.1% same-box,
// bit-identical on C1 and C2 full frames (profiles/r06/ab_unroll.txt). RKF45 keeps the chain
// (C3 -1.4%, C5 neutral in round 3); k_path and the HUGE redo always select.
// The zero-acceleration paths (rotation_trig: C4, C5) keep it too, and form the rotation of
// state[2]'s sin, cos for the new step size in the same rare branch: a regime change is then
// one test per iteration instead of two.
template <int METHOD, bool SPIN0, bool FAR, bool HUGE>
constexpr bool hcache() {
    return (METHOD == INTEGRATOR_RK4 && !HUGE) ||
           rotation_trig<METHOD, SPIN0, FAR, HUGE>();
}

// Where RK4's h * RN(1/6) is kept beside the cached step size and set with it, in the same rare
// branch: the zero-acceleration RK4 path (C4), whose ~60-VALU iteration otherwise re-forms the
// product -- a v_mov_b64 of the constant, an s_nop and the v_mul_f64 -- every time. The same
// product of the same operands, so bit-identical. It costs two more loop-carried registers, so
// it is kept to the path whose listing shows the product: the a = 0 iterations (C1, C2: ~300
// VALU each) keep the inline form.
template <int METHOD, bool SPIN0, bool FAR, bool HUGE>
constexpr bool h6cache() {
    return METHOD == INTEGRATOR_RK4 && rotation_trig<METHOD, SPIN0, FAR, HUGE>();
}

// One pass of integrate_photon_path's loop body (raytracer.c:517-665) plus, with DISK, the
// on-the-fly form of trace_ray's segment scan. Returns the termination, or T_NONE.
// hs: the step sizes in registers (k_trace), or NULL to read them from the scene.
// MASK (k_trace's wave-uniform trip, exit_masks): the return value is the WAVE's mask of lanes
// whose ray ends here -- the exit compares, each its own ballot, ORed as scalars -- and a disk
// hit is noted in the sign bit of R.k, where the step-budget compare (unsigned) sees it; the
// caller forms the termination on the trip's exit edge (exit_term). The iteration itself is the
// same arithmetic either way.
// SKY (k_trace's sky instantiations): the point the iteration started from, p_{k-1}, is kept in
// *ch (Chord). A lane runs no iteration after the one that ends its ray
// (the wave-uniform trips leave on the iteration in which any lane stops, the predicated ones
// skip a lane that stopped), so at the exit it is the terminating iteration's.
template <int METHOD, bool DISK, bool SPIN0, bool FAR, bool HUGE, bool ACC = false,
          bool MASK = false, bool SKY = false>
__device__ __forceinline__ std::conditional_t<MASK, unsigned long long, int> ray_iterate(
    Ray_& R, const Scene& sc, Counters& n, const HSel hs, Chord* ch = nullptr) {
    static_assert(!MASK || (DISK && METHOD == INTEGRATOR_RK4), "MASK: every iteration moves");
    Counters* const hc = HUGE ? nullptr : &n;
    // Instantiations with repair_at_refill() run the recovery once, when the ray is loaded:
    // there a finite state stays finite.
    if (!repair_at_refill<METHOD, FAR, HUGE>()) state_repair(R, hc);
    // step schedule (:556-571), written as selects so the first true test wins; fmin(h, 0.1)
    // is folded into the values (host)
    const double r = R.y[1];
    double h, h6 = 0.0;
    if constexpr (hcache<METHOD, SPIN0, FAR, HUGE>()) {
        // the size is cached per ray with the r interval it holds on (Scene h_lo / h_hi): a ray
        // changes regime at most three times, so each iteration is two compares instead of the
        // three compares and three 64-bit selects of the chain (NaN r: always re-selected,
        // giving the chain's h_far)
        if (__builtin_expect(!(r >= R.h_lo && r < R.h_hi), 0)) {
            int k = 0;
            k = (r < sc.rs_x15) ? 1 : k;
            k = (r < sc.rs_x5) ? 2 : k;
            k = (r < sc.rs_x2_5) ? 3 : k;
            R.h = k == 0 ? hs.far_ : (k == 1 ? hs.r15 : (k == 2 ? hs.r5 : hs.r2_5));
            // (indexed by the per-lane k these are vector loads from the kernel-argument segment,
            // in this rare branch only; selects of the eight bounds as register values instead
            // measured C4 +-0, C5 -1.5% same-box -- more SGPR spills around the loop --
            // profiles/r05/ab_session_l.txt)
            R.h_lo = sc.h_lo[k];
            R.h_hi = sc.h_hi[k];
            if constexpr (rotation_trig<METHOD, SPIN0, FAR, HUGE>()) {
                // the nominal increment of state[2] at this step size: h/6 * ((v + 2v) + 2v) + v
                // (rk4_step) or h * sum5 (rkf45_attempt), v = state[5] (constant here). |d| <
                // pi/4 for every ray k_trace keeps in these instantiations (|v| <
                // Scene.rot_vmax, checked at refill; any other ray is re-traced by the HUGE
                // pass, which advances its trig directly).
                double d;
                if (METHOD == INTEGRATOR_RK4) {
                    double a = R.y[5];
                    a = rk4_acc(a, R.y[5]);
                    a = rk4_acc(a, R.y[5]);
                    R.h6 = R.h * (1.0 / 6.0);
                    d = R.h6 * (a + R.y[5]);
                } else {
                    d = R.h * R.zs[5];
                }
                rotation_coeffs(d, R.cd_sd, R.cd_cm1);
            }
        }
        // h formed at the branch's join: left visible, the compiler sank the step's first uses
        // of h into both arms, and the rare re-select became an if/else diamond (s_xor +
        // s_andn2_saveexec per iteration). C4 SALU 145 -> 137 M per launch, C5 +2%,
        // bit-identical (profiles/r04/session_ad)
        // (the barrier on the carried value itself: on a copy of it, it cost a v_mov_b64 and an
        // s_nop in every iteration)
        asm volatile("" : "+v"(R.h));
        h = R.h;
        if constexpr (h6cache<METHOD, SPIN0, FAR, HUGE>()) {
            asm volatile("" : "+v"(R.h6));
            h6 = R.h6;
        }
    } else {
        h = hs.far_;
        h = (r < sc.rs_x15) ? hs.r15 : h;
        h = (r < sc.rs_x5) ? hs.r5 : h;
        h = (r < sc.rs_x2_5) ? hs.r2_5 : h;
    }
    bool moved = true;
    if (METHOD != INTEGRATOR_RK4) n.iters++;  // RK4: counted at termination (k_trace)
    Trig1 tr{R.y[1], R.s1, R.c1};
    const double a2 = R.y[2], a3 = R.y[3];
    constexpr bool HS = hoist_sums<METHOD, SPIN0, FAR, HUGE>();
    if (METHOD == INTEGRATOR_RK4) {
        if (!h6cache<METHOD, SPIN0, FAR, HUGE>()) h6 = h * (1.0 / 6.0);
        rk4_step<SPIN0, FAR, HUGE, HS>(R.y, h, h6, sc, R.far_ok, n, tr, R.zs);
    } else if (METHOD == INTEGRATOR_RKF45) {
        moved = rkf45_attempt<SPIN0, FAR, HUGE, HS, ACC>(R.y, h, sc, R.far_ok, n, tr, R.zs);
    } else {
        moved = false;  // LEAPFROG / YOSHIDA: "not implemented", state unchanged (:616-624)
    }
    double x, y, z;
    if (moved) {
        // sin, cos of state[1] feed only the a = 0 accelerations (rhs); the Kerr branch
        // (a != 0, accelerations 0) never reads them, and the compiler keeps a dead
        // loop-carried advance alive otherwise (C5: 45 instructions of the loop)
        if constexpr (SPIN0 && METHOD == INTEGRATOR_RK4) {
            // from stage 4's theta, sin, cos (rk4_step left them in tr), a second-order distance
            // away: one coefficient (shift_chain). The carried pair passes through two shifts
            // per iteration, stage 4's and this one.
            double s1, c1;
            shift_chain<1>(tr.a, tr.s, tr.c, R.y[1], s1, c1, hc);
            R.s1 = s1;
            R.c1 = c1;
        } else if (SPIN0) {
            trig_advance(tr.a, R.y[1], R.s1, R.c1, hc);
        }
        if constexpr (rotation_trig<METHOD, SPIN0, FAR, HUGE>()) {
            // (the rotation for this step size was formed with it, above)
            const double s0 = R.s2, c0 = R.c2;
            R.s2 = __builtin_fma(c0, R.cd_sd, __builtin_fma(s0, R.cd_cm1, s0));
            R.c2 = __builtin_fma(-s0, R.cd_sd, __builtin_fma(c0, R.cd_cm1, c0));
        } else {
            trig_advance(a2, R.y[2], R.s2, R.c2, hc);
        }
        // on the zero-acceleration Kerr paths state[3] never changes (zero_accel): its sin,
        // cos stay as they are
        if (!zero_accel<SPIN0, FAR>()) trig_advance(a3, R.y[3], R.s3, R.c3, hc);
    }
    sph2cart_t(R.y[1], R.s2, R.c2, R.s3, R.c3, x, y, z);
    const double ox = R.px, oy = R.py, oz = R.pz;
    R.dist += seg_len<HUGE>(x - ox, y - oy, z - oz);
    if constexpr (SKY) {
        ch->x = ox;
        ch->y = oy;
        ch->z = oz;
    }
    R.px = x;
    R.py = y;
    R.pz = z;
    R.k++;
    if constexpr (!DISK) {
        // exits in the reference's order as early returns (without a disk test they are a
        // short chain of rare branches; the select form below measured -0.9% on C5,
        // profiles/r03_ab_kernel.txt)
        if (R.y[1] <= sc.rs_x1_05) return T_HORIZON;
        if (R.dist >= sc.max_dist) return T_MAXDIST;
        if (!moved) {  // fixed point (below)
            R.k = sc.max_steps;
            return T_MAXSTEPS;
        }
        return R.k >= sc.max_steps ? T_MAXSTEPS : T_NONE;
    } else {
        // the exits as selects (the reference's order: disk, horizon, distance, fixed point,
        // step budget; a disk hit overrides the others below)
        // (as three selects, lowest priority first: the nested form compiled to exec-mask
        // branches)
        int term = T_NONE;
        if constexpr (!MASK) {
            term = (R.k >= sc.max_steps) ? T_MAXSTEPS : T_NONE;
            term = (R.dist >= sc.max_dist) ? T_MAXDIST : term;
            term = (R.y[1] <= sc.rs_x1_05) ? T_HORIZON : term;
        }
        // segment k = (p_k, p_{k-1}) is stored and scanned by trace_ray iff k < max_steps
        // (MASK: that test inside the candidates' rare branch -- beside k >= max_steps above it
        // was a second compare of the same operands in every iteration; the barrier keeps the
        // compiler from hoisting it back)
        double qx, qy, qz, num, den;
        if (disk_cand(R, ox, oy, oz, sc, hs.big, num, den) & (MASK || R.k < sc.max_steps)) {
            int kq = R.k;
            if constexpr (MASK) asm volatile("" : "+v"(kq));
            if ((!MASK || kq < sc.max_steps) && disk_decide(R, num, den, sc, qx, qy, qz)) {
                // the ray ends here: the hit point replaces the current point, so no extra
                // loop-carried registers hold it (store_hit reads it from R.px..pz; +0.9% on C2)
                R.px = qx;
                R.py = qy;
                R.pz = qz;
                const double ux = qx - ox, uy = qy - oy, uz = qz - oz;
                R.dist += sqrt_nr((ux * ux + uy * uy) + uz * uz);  // (= len3: sqrt_nr is sqrt here)
                term = T_DISK;
                if constexpr (MASK) R.k |= kStopMark;
            }
        }
        if constexpr (MASK) {
            // a v_cmp's result IS the ballot of its lanes: three compares and two scalar ORs, no
            // 32-bit select and no compare of a code (the ballot of an ORed lane mask came out
            // as a v_cndmask and a v_cmp). 0 < max_steps here, so the unsigned compare is the
            // budget test for a step count and true for one that carries kStopMark.
            R.k |= n.mark;  // (`huge` raised: Counters)
            return __builtin_amdgcn_ballot_w64((unsigned)R.k >= (unsigned)sc.max_steps) |
                   __builtin_amdgcn_ballot_w64(R.dist >= sc.max_dist) |
                   __builtin_amdgcn_ballot_w64(R.y[1] <= sc.rs_x1_05);
        }
        if (!moved && term == T_NONE) {
            // Fixed point: every later iteration repeats this one with p_j = p_{j-1} = p_k.
            // Only the duplicate segment (p_k, p_k) is new, and only if p_k != p_{k-1}.
            if (R.k + 1 < sc.max_steps && (x != ox || y != oy || z != oz) &&
                disk_hit(R, x, y, z, sc, hs.big, qx, qy, qz)) {
                R.px = qx;
                R.py = qy;
                R.pz = qz;
                R.k++;
                R.dist += len3(qx - x, qy - y, qz - z);
                return T_DISK;
            }
            R.k = sc.max_steps;
            return T_MAXSTEPS;
        }
        return term;
    }
}

// fill_hit_info (raytracer.c:299-333) / the disk branch of trace_ray (:728-753)
__device__ __forceinline__ void store_hit(const bhrt_frame_soa& s, int i, const Ray_& R,
                                          int term, const Scene& sc) {
    int result, steps;
    double hx, hy, hz, tdil, sx = 0.0, sy = 0.0, sz = 0.0;
    if (term == T_DISK) {
        result = RAY_DISK;
        steps = R.k;
        hx = R.px;
        hy = R.py;
        hz = R.pz;
        tdil = 1.0 / sqrt(1.0 - sc.rs / len3(R.px, R.py, R.pz));
    } else {
        result = term == T_HORIZON ? RAY_HORIZON
                                   : (term == T_MAXDIST ? RAY_MAX_DISTANCE : RAY_MAX_STEPS);
        steps = term == T_MAXSTEPS ? R.k : R.k - 1;
        hx = R.px;
        hy = R.py;
        hz = R.pz;
        tdil = 1.0 / sqrt(1.0 - sc.rs / R.y[1]);
        if (term == T_MAXDIST) normalize3(R.y[5], R.y6, R.y7, sx, sy, sz);  // state[5..7]
    }
    if (s.result) s.result[i] = result;
    if (s.steps) s.steps[i] = steps;
    if (s.hit_x) s.hit_x[i] = hx;
    if (s.hit_y) s.hit_y[i] = hy;
    if (s.hit_z) s.hit_z[i] = hz;
    if (s.distance) s.distance[i] = R.dist;
    if (s.time_dilation) s.time_dilation[i] = tdil;
    if (s.sky_x) s.sky_x[i] = sx;
    if (s.sky_y) s.sky_y[i] = sy;
    if (s.sky_z) s.sky_z[i] = sz;
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

#include "bhrt_colour.h"

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

__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
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

// integrate_photon_path with a recorded path (one ray, one lane). The output hit goes to
// element 0 of kp.out; the path and the stored-point count to path / d_num.
template <int METHOD, bool SPIN0>
__global__ void k_path(const bhrt_kparams kp, double t0, double ox, double oy, double oz,
                       double dx, double dy, double dz, Vector3D* path, int max_positions,
                       int* d_num, int num_in) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Counters n;
    Ray_ R;
    ray_init_general(R, t0, ox, oy, oz, dx, dy, dz, kp.sc);
    trig_anchor(R);
    int num = num_in;
    if (path && max_positions > 0) {  // :504-507
        path[0].x = R.px;
        path[0].y = R.py;
        path[0].z = R.pz;
        num = 1;
    }
    int term = T_MAXSTEPS;
    if (kp.sc.max_steps > 0) {
        for (;;) {
            const int k_before = R.k;
            term = ray_iterate<METHOD, false, SPIN0, true, true>(R, kp.sc, n, hsel_of(kp.sc));
            // positions of the iterations executed (a fixed-point jump repeats p_k)
            for (int j = k_before; j < R.k && path && num >= 0 && num < max_positions; j++) {
                path[num].x = R.px;
                path[num].y = R.py;
                path[num].z = R.pz;
                num++;
            }
            if (term != T_NONE) break;
        }
    }
    if (d_num) *d_num = num;
    store_hit(kp.out, 0, R, term, kp.sc);
}

// Batched recorded paths (bhrt_api.h bhrt_trace_paths_device): one lane per ray, one wave per
// workgroup, a grid sized to the device whose waves claim runs of 64 consecutive rays from
// kp.ctl[0] until none are left. Every iteration is k_path's own call of ray_iterate -- the
// general, always-select instantiation -- so each point has the single-ray kernel's bits; with
// DISK the same instantiation scans trace_ray's segments on the fly, and R.px..pz holds the hit
// point once it returns T_DISK. The rays' hit records are not written here: a caller that wants
// them gets the trace kernel's own (paths.c), whose multi-iteration trips round a long ray's last
// bits differently from this instantiation (profiles/paths/hits_bits.txt).
// Point j of the full path is the position after iteration j (R.k == j; q_0 the origin). A lane
// keeps the multiples of `every` (next_keep: the next one) and, at its end, the last point if
// that was not one; `slot` counts what it stored, and nothing is stored from max_positions on. A
// fixed-point jump of R.k to max_steps walks the kept indices it passed (one trip per STORED
// point: at most max_positions), never the iterations themselves.
// Store forms (STAGED):
//  direct  the lane writes its 24 B point (12 B of xyz32) where it is produced: 64 partial lines
//          per wave and iteration, merged in L2 with the lane's next points;
//  staged  the lane appends to its ring of BHRT_PATHS_RING points in LDS (slots [rbase, rbase +
//          pend) of its row, always consecutive). When any lane's ring is full, and at the end of
//          the claim, the wave flushes: per lane with pending points, a half-wave's consecutive
//          lanes write that lane's run double by double, two source lanes per store instruction,
//          each run 24 B .. 192 B contiguous. A lane whose ring is full before the flush (the
//          stored points of a fixed-point jump) writes the rest directly: other slots, so no order
//          is needed between the two.
constexpr int kRingDoubles = BHRT_PATHS_RING * 3;
constexpr int kRingStride = kRingDoubles + 1;  // odd: lanes' rings start on different LDS banks
static_assert(kRingDoubles <= 32, "a half-wave writes one lane's ring");

// Occupancy: the register budget is the compiler's: compiled for 4 or 3 waves per SIMD the
// direct form lost 6% on C2 and 13-14% on C4.
template <int METHOD, bool DISK, bool SPIN0, bool STAGED>
__global__ __launch_bounds__(64) void k_paths(const bhrt_kparams kp, const bhrt_paths_k pk) {
    __shared__ double ring[STAGED ? 64 * kRingStride : 1];
    const int lane = threadIdx.x;
    const size_t P = (size_t)pk.max_positions;
    const long long every = pk.every;
    double* const xyz = reinterpret_cast<double*>(pk.out.xyz);
    float* const xyz32 = pk.out.xyz32;
    const bool record = xyz != nullptr || xyz32 != nullptr;
    if (lane == 0) atomicMax(kp.ctl + 8, ~(unsigned long long)wall_clock64());
    Counters n;
    const HSel hsel = hsel_of(kp.sc);
    for (;;) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(kp.ctl, 64ull);
        base = __shfl(base, 0);
        if (base >= (unsigned long long)kp.n) break;
        const int i = (int)base + lane;
        const bool live = i < kp.n;
        const size_t row = (size_t)(live ? i : 0) * P;  // element index of the ray's slot 0
        Ray_ R;
        int term = T_MAXSTEPS;
        size_t slot = 0;           // points stored (or counted, without a path output)
        long long next_keep = 0;   // the next path index that is kept
        int pend = 0;              // staged: points in the lane's ring
        size_t rbase = 0;          // staged: the slot of the ring's first point
        // the point (x, y, z) is kept: into slot `slot` (the caller checked slot < P)
        auto emit = [&](double x, double y, double z) {
            if (record) {
                if (STAGED && pend < BHRT_PATHS_RING) {
                    if (pend == 0) rbase = slot;
                    double* q = ring + lane * kRingStride + pend * 3;
                    q[0] = x;
                    q[1] = y;
                    q[2] = z;
                    pend++;
                } else {
                    const size_t e = (row + slot) * 3;
                    if (xyz) {
                        xyz[e] = x;
                        xyz[e + 1] = y;
                        xyz[e + 2] = z;
                    }
                    if (xyz32) {
                        xyz32[e] = (float)x;
                        xyz32[e + 1] = (float)y;
                        xyz32[e + 2] = (float)z;
                    }
                }
            }
            slot++;
            next_keep += every;
        };
        auto flush = [&]() {  // wave-uniform: every lane calls it
            if (!STAGED) return;
            __syncthreads();  // (one wave: the rings' LDS writes have landed)
            unsigned long long m = __ballot(pend > 0);
            const int half = lane >> 5, t = lane & 31;
            while (m) {
                const int l0 = __ffsll((long long)m) - 1;
                m &= m - 1;
                int l1 = -1;
                if (m) {
                    l1 = __ffsll((long long)m) - 1;
                    m &= m - 1;
                }
                const int l = half ? l1 : l0;
                const int src = l < 0 ? l0 : l;
                const int cnt = __shfl(pend, src);
                const unsigned long long e0 =
                    __shfl((unsigned long long)((row + rbase) * 3), src);
                if (l >= 0 && t < cnt * 3) {
                    const double v = ring[src * kRingStride + t];
                    if (xyz) xyz[(size_t)e0 + t] = v;
                    if (xyz32) xyz32[(size_t)e0 + t] = (float)v;
                }
            }
            __syncthreads();  // the rings are free again
            pend = 0;
        };
        bool run = false;
        if (live) {
            const Ray ray = kp.rays[i];
            ray_init_general(R, 0.0, ray.origin.x, ray.origin.y, ray.origin.z, ray.direction.x,
                             ray.direction.y, ray.direction.z, kp.sc);
            trig_anchor(R);
            emit(R.px, R.py, R.pz);  // q_0 (:504-507); max_positions >= 1
            run = kp.sc.max_steps > 0;
        }
        while (__ballot(run) != 0ull) {
            if (run) {
                const int k_before = R.k;
                term = ray_iterate<METHOD, DISK, SPIN0, true, true>(R, kp.sc, n, hsel);
                if (DISK && term == T_DISK && R.k - k_before == 2) {
                    // a stuck ray whose duplicate segment hits (ray_iterate's fixed point): the
                    // stuck point is q_{k-1} -- the unchanged state's position -- and the hit q_k
                    if (next_keep == (long long)R.k - 1 && slot < P) {
                        double x, y, z;
                        sph2cart_t(R.y[1], R.s2, R.c2, R.s3, R.c3, x, y, z);
                        emit(x, y, z);
                    }
                }
                // indices (k_before, R.k] all hold the current point; next_keep > k_before
                while (next_keep <= (long long)R.k && slot < P) emit(R.px, R.py, R.pz);
                if (term != T_NONE) {
                    // the end of the ray, unless it was just kept (next_keep - every: the last
                    // kept index where nothing was truncated; a truncated ray stores no more)
                    if (next_keep - every != (long long)R.k && slot < P) emit(R.px, R.py, R.pz);
                    run = false;
                }
            }
            if (STAGED && __ballot(pend == BHRT_PATHS_RING) != 0ull) flush();
        }
        flush();
        if (live) {
            if (pk.out.count) pk.out.count[i] = (int)slot;
            n.rays++;
            if (METHOD == INTEGRATOR_RK4) n.iters += R.k;  // (counted at termination, as k_trace)
        }
    }
    const unsigned long long s0 = wave_sum(n.rays), s1 = wave_sum(n.iters), s2 = wave_sum(n.full),
                             s3 = wave_sum(n.far_), s4 = wave_sum(n.kerr);
    if (lane == 0) {
        atomicMax(kp.ctl + 9, (unsigned long long)wall_clock64());
        if (s0) atomicAdd(kp.ctl + 1, s0);
        if (s1) atomicAdd(kp.ctl + 2, s1);
        if (s2) atomicAdd(kp.ctl + 3, s2);
        if (s3) atomicAdd(kp.ctl + 4, s3);
        if (s4) atomicAdd(kp.ctl + 5, s4);
    }
}

// Both forms of the RKF45 accept test (rkf45_accept) on given operands: case i has six
// components err[6i..6i+5], scale[6i..6i+5] and tolerance tol[i]; out[2i] = the fast form's
// decision, out[2i+1] = the literal quotient's.
__global__ void k_check_accept(const double* err, const double* scale, const double* tol, int n,
                               int* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double e[6], s[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        e[c] = err[6 * i + c];
        s[c] = scale[6 * i + c];
    }
    out[2 * i] = rkf45_accept<true>(e, s, tol[i]);
    out[2 * i + 1] = rkf45_accept<false>(e, s, tol[i]);
}

// The trace loop's disk decision (disk_hit) on given operands: case i is the point p[3i..3i+2],
// the direction d[3i..] and the "normal" n[3i..] (the previous path point); out[i] = the
// decision against the thresholds in_sq, out_sq (Scene disk_in_sq / disk_out_sq). One wave per
// workgroup, so lanes of either form share a wave as they do in the loop.
__global__ void k_check_disk_hit(const double* p, const double* d, const double* nrm, int n,
                                 double in_sq, double out_sq, int* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Scene sc{};
    sc.disk_in_sq = in_sq;
    sc.disk_out_sq = out_sq;
    Ray_ R{};
    R.px = p[3 * i];
    R.py = p[3 * i + 1];
    R.pz = p[3 * i + 2];
    R.dx = d[3 * i];
    R.dy = d[3 * i + 1];
    R.dz = d[3 * i + 2];
    const HSel hs = hsel_of(sc);
    double qx, qy, qz;
    out[i] = disk_hit(R, nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], sc, hs.big, qx, qy, qz);
}

// The root seg_len takes of its sum (sqrt_nr1) on given arguments
__global__ void k_check_seg_len(const double* x, int n, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = sqrt_nr1(x[i]);
}

// The shared reciprocal of an RK4 stage pair (stage_x, pair_rcp) on given operands: case i is
// (rc_a, st_a, rc_b, st_b) = in[4i..4i+3]; out[5i..5i+3] = 1 / rc_a, 1 / st_a, 1 / rc_b, 1 / st_b
// as the stages form them (accel_fast's yr2, ys2 times -1/2, exact) and out[5i+4] = the pair's
// range test (1: both stages use these quotients; 0: both take the literal form instead).
// huge: with the rc < 1e150 test of the HUGE redo pass and k_path.
__global__ void k_check_pair_rcp(const double* in, int n, int huge, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    StageOps a, b;
    a.rc = in[4 * i];
    a.st = in[4 * i + 1];
    b.rc = in[4 * i + 2];
    b.st = in[4 * i + 3];
    a.ct = b.ct = 0.0;
    if (huge) {
        stage_x<true>(a);
        stage_x<true>(b);
    } else {
        stage_x<false>(a);
        stage_x<false>(b);
    }
    double wa, wb;
    const bool ok = pair_rcp(a, b, wa, wb);
    out[5 * i] = -0.5 * (a.st * wa);
    out[5 * i + 1] = -0.5 * (a.rc * wa);
    out[5 * i + 2] = -0.5 * (b.st * wb);
    out[5 * i + 3] = -0.5 * (b.rc * wb);
    out[5 * i + 4] = ok ? 1.0 : 0.0;
}

// A chained shift (shift_chain) on given operands: case i is (a, s0, c0, x) = in[4i..4i+3], site 0
// stage 3 from stage 2's angle (two coefficients, |x - a| <= 1/64), site 1 the advance of
// state[1] from stage 4's angle (one coefficient, |x - a| <= 2^-10). out[5i..5i+1] = sin, cos of x
// as the chained form gives them, out[5i+2..5i+3] as shift_or_eval does from the same operands,
// out[5i+4] = 1 if the lane kept the short polynomials, 0 if it redid the shift. Direct
// evaluations take the redo pass's form (no counters: the library sincos above 2^20).
__global__ void k_check_shift_chain(const double* in, int n, int site, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = in[4 * i], s0 = in[4 * i + 1], c0 = in[4 * i + 2], x = in[4 * i + 3];
    double s, c, s_ref, c_ref;
    const bool fast = site == 0 ? shift_chain<2>(a, s0, c0, x, s, c, nullptr)
                                : shift_chain<1>(a, s0, c0, x, s, c, nullptr);
    shift_or_eval(a, s0, c0, x, s_ref, c_ref, nullptr);
    out[5 * i] = s;
    out[5 * i + 1] = c;
    out[5 * i + 2] = s_ref;
    out[5 * i + 3] = c_ref;
    out[5 * i + 4] = fast ? 1.0 : 0.0;
}

// A high-word guard (all_below_2) beside the exact test it filters for, on given operands.
// kind 0, the one guard built: accel_fast's plain-value test of a stage's three accelerations
// a[3i..3i+2] (b is not read). out[2i] = the filter's answer (all_below_2), out[2i+1] = the exact
// test's (every |a| <= 10, NaN failing).
__global__ void k_check_guard_words(const double* a, const double* /*b*/, int n, int* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d3 = a[3 * i], d4 = a[3 * i + 1], d5 = a[3 * i + 2];
    out[2 * i] = all_below_2(d3, d4, d5);
    out[2 * i + 1] = (int)(fabs(d3) <= 10.0) & (int)(fabs(d4) <= 10.0) & (int)(fabs(d5) <= 10.0);
}

// ---- launch plumbing --------------------------------------------------------------------
// Launch geometry is cached per device: a process may drive several devices (bhrt_render_frame
// splits a frame over every visible one) from several host threads. Every cached value is a
// pure function of (device, kernel), so concurrent first calls may both compute it and store
// the same value; the atomics make that race-free without a lock on the launch path.
constexpr int kMaxDev = 64;
std::atomic<int> g_cus[kMaxDev];

int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) dev = 0;
    return dev;
}

int device_cus(int dev) {
    int cus = g_cus[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            cus <= 0)
            cus = 256;
        g_cus[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// resident workgroups of `lanes` lanes of kernel fn on device dev (the persistent grid)
int resident_blocks(const void* fn, int dev, int lanes = 256) {
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, lanes, 0);
    if (per_cu <= 0) per_cu = 1;
    return device_cus(dev) * per_cu;
}

// grid of a grid-stride elementwise kernel over n items (at most one resident wave of blocks)
int grid_for(const void* fn, int n) {
    long blocks = ((long)n + 255) / 256;
    const long cap = resident_blocks(fn, current_device());
    if (blocks > cap) blocks = cap;
    return blocks < 1 ? 1 : (int)blocks;
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

template <int METHOD>
void launch_path(const bhrt_kparams& kp, const double* o4, const double* d3, Vector3D* d_path,
                 int max_positions, int* d_num, int num_in, hipStream_t st) {
    if (kp.sc.spin0)
        k_path<METHOD, true><<<1, 64, 0, st>>>(kp, o4[0], o4[1], o4[2], o4[3], d3[0], d3[1], d3[2],
                                               d_path, max_positions, d_num, num_in);
    else
        k_path<METHOD, false><<<1, 64, 0, st>>>(kp, o4[0], o4[1], o4[2], o4[3], d3[0], d3[1],
                                                d3[2], d_path, max_positions, d_num, num_in);
}

// k_paths on a grid of the device's resident one-wave workgroups, at most one per 64 rays
template <int METHOD, bool DISK, bool SPIN0>
int launch_paths_t(const bhrt_kparams& kp, const bhrt_paths_k& pk, hipStream_t st, hipEvent_t e0,
                   hipEvent_t e1) {
    void (*const fn)(const bhrt_kparams, const bhrt_paths_k) =
        pk.staged ? &k_paths<METHOD, DISK, SPIN0, true> : &k_paths<METHOD, DISK, SPIN0, false>;
    long blocks = resident_blocks(reinterpret_cast<const void*>(fn), current_device(), 64);
    const long runs = ((long)kp.n + 63) / 64;
    if (blocks > runs) blocks = runs;
    if (e0) (void)hipEventRecord(e0, st);
    fn<<<(unsigned)blocks, 64, 0, st>>>(kp, pk);
    if (e1) (void)hipEventRecord(e1, st);
    return (int)hipGetLastError();
}

template <int METHOD>
int launch_paths_m(const bhrt_kparams& kp, const bhrt_paths_k& pk, hipStream_t st, hipEvent_t e0,
                   hipEvent_t e1) {
    if (kp.sc.has_disk)
        return kp.sc.spin0 ? launch_paths_t<METHOD, true, true>(kp, pk, st, e0, e1)
                           : launch_paths_t<METHOD, true, false>(kp, pk, st, e0, e1);
    return kp.sc.spin0 ? launch_paths_t<METHOD, false, true>(kp, pk, st, e0, e1)
                       : launch_paths_t<METHOD, false, false>(kp, pk, st, e0, e1);
}

}  // namespace

extern "C" int bhrt_launch_paths(const bhrt_kparams* kp, const bhrt_paths_k* pk, void* stream,
                                 void* ev0, void* ev1) {
    if (kp->n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(ev0), e1 = static_cast<hipEvent_t>(ev1);
    switch (kp->sc.method) {
    case INTEGRATOR_RK4: return launch_paths_m<INTEGRATOR_RK4>(*kp, *pk, st, e0, e1);
    case INTEGRATOR_RKF45: return launch_paths_m<INTEGRATOR_RKF45>(*kp, *pk, st, e0, e1);
    default: return launch_paths_m<INTEGRATOR_LEAPFROG>(*kp, *pk, st, e0, e1);  // no-op integrators
    }
}

extern "C" int bhrt_launch_sky(const bhrt_sky_k* sky, const double* d_dirs, int n, double* d_rgb,
                               void* stream) {
    if (n <= 0) return 0;
    k_sky_lookup<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(*sky, d_dirs, n,
                                                                               d_rgb);
    return (int)hipGetLastError();
}

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

extern "C" __attribute__((visibility("default"))) int bhrt_check_rkf45_accept(
    const double* d_err, const double* d_scale, const double* d_tol, int n, int* d_out,
    void* stream) {
    if (n <= 0) return 0;
    k_check_accept<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(
        d_err, d_scale, d_tol, n, d_out);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int bhrt_check_disk_hit(
    const double* d_p, const double* d_d, const double* d_n, int n, double in_sq, double out_sq,
    int* d_out, void* stream) {
    if (n <= 0) return 0;
    k_check_disk_hit<<<(n + 63) / 64, 64, 0, static_cast<hipStream_t>(stream)>>>(
        d_p, d_d, d_n, n, in_sq, out_sq, d_out);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int bhrt_check_seg_len(const double* d_x, int n,
                                                                         double* d_out,
                                                                         void* stream) {
    if (n <= 0) return 0;
    k_check_seg_len<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(d_x, n, d_out);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int bhrt_check_pair_rcp(const double* d_in, int n,
                                                                        int huge, double* d_out,
                                                                        void* stream) {
    if (n <= 0) return 0;
    k_check_pair_rcp<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(d_in, n, huge,
                                                                                   d_out);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int bhrt_check_shift_chain(
    const double* d_in, int n, int site, double* d_out, void* stream) {
    if (n <= 0) return 0;
    if (site != 0 && site != 1) return (int)hipErrorInvalidValue;
    k_check_shift_chain<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(d_in, n, site,
                                                                                      d_out);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int bhrt_check_guard_words(
    const double* d_a, const double* d_b, int n, int kind, int* d_out, void* stream) {
    if (n <= 0) return 0;
    if (kind != 0) return (int)hipErrorInvalidValue;
    k_check_guard_words<<<(n + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(d_a, d_b, n,
                                                                                      d_out);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_path(const bhrt_kparams* kp, const double* o4, const double* d3,
                                Vector3D* d_path, int max_positions, int* d_num, int num_in,
                                void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (kp->sc.method) {
    case INTEGRATOR_RK4:
        launch_path<INTEGRATOR_RK4>(*kp, o4, d3, d_path, max_positions, d_num, num_in, st);
        break;
    case INTEGRATOR_RKF45:
        launch_path<INTEGRATOR_RKF45>(*kp, o4, d3, d_path, max_positions, d_num, num_in, st);
        break;
    default:
        launch_path<INTEGRATOR_LEAPFROG>(*kp, o4, d3, d_path, max_positions, d_num, num_in, st);
        break;
    }
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_ss_rays(const bhrt_ss_rays_k* k, void* stream) {
    if (k->n <= 0 || k->sample < 0) return 0;
    k_ss_rays<<<(unsigned)(((long)k->n + 255) / 256), 256, 0,
                static_cast<hipStream_t>(stream)>>>(*k);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_ss_resolve(const bhrt_ss_resolve_k* k, void* stream) {
    if (k->n <= 0 || k->samples <= 0) return 0;
    k_ss_resolve<<<(unsigned)(((long)k->n + 255) / 256), 256, 0,
                   static_cast<hipStream_t>(stream)>>>(*k);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_ad_rays(const bhrt_ad_rays_k* k, void* stream) {
    if (k->n <= 0 || k->first < 0) return 0;
    k_ad_rays<<<(unsigned)(((long)k->n + 255) / 256), 256, 0,
                static_cast<hipStream_t>(stream)>>>(*k);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_ad_edges(const bhrt_ad_edges_k* k, void* stream) {
    if (k->n <= 0 || k->base <= 0) return 0;
    k_ad_edges<<<(unsigned)(((long)k->n + 255) / 256), 256, 0,
                 static_cast<hipStream_t>(stream)>>>(*k);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_ad_resolve(const bhrt_ad_resolve_k* k, void* stream) {
    if (k->n <= 0 || k->base <= 0) return 0;
    k_ad_resolve<<<(unsigned)(((long)k->n + 255) / 256), 256, 0,
                   static_cast<hipStream_t>(stream)>>>(*k);
    return (int)hipGetLastError();
}

// (exact grids with a tail guard; n <= INT_MAX, so the workgroup count fits an unsigned)
extern "C" int bhrt_launch_ta_blend(const bhrt_ta_blend_k* k, void* stream) {
    if (k->n <= 0 || (k->stride != 3 && k->stride != 4)) return 0;
    k_ta_blend<<<(unsigned)((k->n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(*k);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_ta_edges(const bhrt_ta_edges_k* k, void* stream) {
    if (k->n <= 0 || k->width <= 0 || k->n != (long)k->width * k->height) return 0;
    k_ta_edges<<<(unsigned)((k->n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(*k);
    return (int)hipGetLastError();
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
