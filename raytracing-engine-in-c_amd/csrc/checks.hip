// checks.hip -- test-only kernels: single pieces of bhrt_trace_core.h's arithmetic run on given
// operands, and their exported bhrt_check_* entry points (called by the GPU tests through ctypes;
// no product path launches them).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bhrt_kernel.h"

#pragma clang fp contract(fast)

namespace {

#include "bhrt_trace_core.h"

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

}  // namespace

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
