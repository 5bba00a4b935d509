// bhrt_trace_core.h -- the device core of the geodesic ray tracer: the arithmetic helpers, the
// right-hand side, the RK4 and RKF45 steps, the ray state and its set-up, the disk test, one
// iteration of a ray (ray_iterate) and the hit record, as device functions shared by the kernels of
// geodesic.hip (k_init, k_trace, k_colour), paths.hip (k_path, k_paths), frames.hip (the camera
// directions and colour stores of the frame passes) and checks.hip (k_check_*). Included inside
// the including file's unnamed namespace, after <hip/hip_runtime.h>, <type_traits>,
// "bhrt_kernel.h" and the file-level `#pragma clang fp contract(fast)`. The text below is
// geodesic.hip's own, moved here unchanged: every function is the same operation sequence
// wherever it is inlined. What only one unit uses is in that unit.

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

// Narrow-first shifts from the FAR anchor. Four more shifts of the RK4
// a = 0 iteration -- stage 2's and stage 4's theta and the advances of state[2] and state[3] --
// start from the iteration's own start, a first-order distance away, and ran shift_or_eval's
// three coefficients. Three of them take shift_chain<2>'s two coefficients on |delta| <= 1/64
// first (-3 VALU each); a lane beyond the bound redoes the shift with shift_or_eval, as at the
// chained sites. On camera B every such lane is in the first seven iterations of its ray
// (tools/shift_deltas.py --ages, profiles/nursery/shift_ages.txt), and a wave takes fresh rays
// about ten times in its ~3200 iterations (profiles/nursery/wave_stamps_parent.txt), so the redo
// runs in ~2% of the wave-iterations: C2 +1.4%, C1 +2.4% same-box.
// The advance of state[2] keeps the wide form first: with it narrow too camera B gains +2.6%,
// but the far camera V's frame of five-iteration rays, every one beyond the bound at that site,
// loses 3-5% -- also where a wave with no lane inside the bound skips the short polynomials, so
// it is not their arithmetic -- and gains 7% without it (profiles/nursery/ab_parent_vs_new.txt).
// The choice is a pure function of the lane's operands, in every instantiation alike (camera
// frames, ray arrays, k_path, k_paths, the HUGE redo, the check kernels), so a ray's bits never
// depend on its age, its wave-mates or the kernel that traces it.
// BHRT_NARROW_SITES (A/B builds): bit 0 stage 2, bit 1 stage 4, bit 2 the advance of state[2],
// bit 3 the advance of state[3]; 0 is the parent's iteration.
#ifndef BHRT_NARROW_SITES
#define BHRT_NARROW_SITES 11
#endif
constexpr int kNC2 = (BHRT_NARROW_SITES & 1) ? 2 : 0, kNC4 = (BHRT_NARROW_SITES & 2) ? 2 : 0;
constexpr bool kNarrowY2 = (BHRT_NARROW_SITES & 4) != 0, kNarrowY3 = (BHRT_NARROW_SITES & 8) != 0;

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
            stage_ops<FAR, HUGE, kNC2>(y20, y21, far2, sc, n, tr, o2);
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
            stage_ops<FAR, HUGE, kNC4>(y40, y41, far4, sc, n, tr, o4);
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
// NARROW: two coefficients on |x - a| <= 1/64 first (shift_chain<2>, BHRT_NARROW_SITES).
template <bool NARROW = false>
__device__ __forceinline__ void trig_advance(double a, double x, double& s, double& c,
                                             Counters* hc) {
    double s1, c1;
    if constexpr (NARROW)
        shift_chain<2>(a, s, c, x, s1, c1, hc);
    else
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
    // the RK4 a = 0 iteration's advances of state[2], state[3]: BHRT_NARROW_SITES
    constexpr bool A0 = SPIN0 && METHOD == INTEGRATOR_RK4;
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
            trig_advance<A0 && kNarrowY2>(a2, R.y[2], R.s2, R.c2, hc);
        }
        // on the zero-acceleration Kerr paths state[3] never changes (zero_accel): its sin,
        // cos stay as they are
        if (!zero_accel<SPIN0, FAR>()) trig_advance<A0 && kNarrowY3>(a3, R.y[3], R.s3, R.c3, hc);
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

#include "bhrt_colour.h"

__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
