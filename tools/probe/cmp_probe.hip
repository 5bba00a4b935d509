// Issue cost of a guard compare beside a stream of f64 FMAs on gfx950. Each wave runs a loop of
// 16 independent v_fma_f64 (one per accumulator) with k compares spread among them, k = 0, 2, 4,
// and times it with the wave's clock (s_memtime). The compare is, in turn,
//   f64   v_cmp_le_f64 s[..], |x|, s[..]          today's guard
//   f32   v_cmp_lt_f32 s[..], |hi|, s             the same guard on the operand's high word
//   or3   v_or3_b32 of three high words + one v_cmp_lt_f32 (the merged plain-value test)
// at 1 and at 4 waves per SIMD (one workgroup of 256 or 1024 lanes on one CU). Reported: cycles
// per loop pass of the slowest wave, and SIMD cycles (wave cycles / waves per SIMD) per added
// compare (or3: per added PAIR of instructions) against the k = 0 stream at the same occupancy.
// Diagnostic only.
//   hipcc --offload-arch=gfx950 -O3 tools/probe/cmp_probe.hip -o cmp_probe && ./cmp_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

enum Kind { F64 = 0, F32 = 1, OR3 = 2 };

// operands: 0-15 accumulators, 16 compare mask (SGPR pair), 17 a scratch word, 18 x, 19 y,
// 20 f64 threshold (SGPR pair), 21 f32 threshold (SGPR), 22-24 three 32-bit words
#define FMA4(a, b, c, d)                       \
    "v_fma_f64 %" #a ", %" #a ", %18, %19\n"   \
    "v_fma_f64 %" #b ", %" #b ", %18, %19\n"   \
    "v_fma_f64 %" #c ", %" #c ", %18, %19\n"   \
    "v_fma_f64 %" #d ", %" #d ", %18, %19\n"
#define C_F64(acc) "v_cmp_le_f64 %16, |%" #acc "|, %20\n"
#define C_F32(w) "v_cmp_lt_f32 %16, |%" #w "|, %21\n"
#define C_OR3(p, q, r) "v_or3_b32 %17, %" #p ", %" #q ", %" #r "\nv_cmp_lt_f32 %16, |%17|, 2.0\n"
#define OPERANDS                                                                                 \
    : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]),        \
      "+v"(a[7]), "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]),    \
      "+v"(a[14]), "+v"(a[15]), "+s"(m), "+v"(t)                                                 \
    : "v"(x), "v"(y), "s"(thr), "s"(thr32), "v"(w0), "v"(w1), "v"(w2)
// one pass: 16 FMAs with nothing, or a compare after the second and fourth group, or after each
#define PASS0 FMA4(0, 1, 2, 3) FMA4(4, 5, 6, 7) FMA4(8, 9, 10, 11) FMA4(12, 13, 14, 15)
#define PASS2(c0, c1) FMA4(0, 1, 2, 3) FMA4(4, 5, 6, 7) c0 FMA4(8, 9, 10, 11) FMA4(12, 13, 14, 15) c1
#define PASS4(c0, c1, c2, c3) \
    FMA4(0, 1, 2, 3) c0 FMA4(4, 5, 6, 7) c1 FMA4(8, 9, 10, 11) c2 FMA4(12, 13, 14, 15) c3

template <int KIND, int K>
__global__ __launch_bounds__(1024) void k_stream(double x, double y, double thr, float thr32, int passes,
                         unsigned long long* cyc, double* sink) {
    double a[16];
#pragma unroll
    for (int i = 0; i < 16; i++) a[i] = 1.0 + 0x1p-30 * (threadIdx.x + i);
    float w0 = 0.25f + threadIdx.x, w1 = 0.5f, w2 = 0.75f, t = 0.0f;
    unsigned long long m = 0;
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int p = 0; p < passes; p++) {
        if constexpr (K == 0)
            asm volatile(PASS0 OPERANDS);
        else if constexpr (KIND == F64 && K == 2)
            asm volatile(PASS2(C_F64(0), C_F64(8)) OPERANDS);
        else if constexpr (KIND == F64)
            asm volatile(PASS4(C_F64(0), C_F64(4), C_F64(8), C_F64(12)) OPERANDS);
        else if constexpr (KIND == F32 && K == 2)
            asm volatile(PASS2(C_F32(22), C_F32(23)) OPERANDS);
        else if constexpr (KIND == F32)
            asm volatile(PASS4(C_F32(22), C_F32(23), C_F32(24), C_F32(22)) OPERANDS);
        else if constexpr (K == 2)
            asm volatile(PASS2(C_OR3(22, 23, 24), C_OR3(23, 24, 22)) OPERANDS);
        else
            asm volatile(PASS4(C_OR3(22, 23, 24), C_OR3(23, 24, 22), C_OR3(24, 22, 23),
                               C_OR3(22, 24, 23)) OPERANDS);
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    double s = (double)(m & 1) + t;
#pragma unroll
    for (int i = 0; i < 16; i++) s += a[i];
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    sink[gid] = s;
    if ((threadIdx.x & 63) == 0) cyc[gid >> 6] = t1 - t0;
}

#define CHECK(e)                                                                   \
    do {                                                                           \
        hipError_t err_ = (e);                                                     \
        if (err_ != hipSuccess) {                                                  \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));              \
            return 1;                                                              \
        }                                                                          \
    } while (0)

constexpr int kPasses = 20000;
constexpr int kMaxLanes = 1024;

template <int KIND, int K>
static int run(int lanes, unsigned long long* d_cyc, double* d_sink, double* per_pass) {
    std::vector<unsigned long long> cyc(kMaxLanes / 64);
    double best = 1e300;
    for (int rep = 0; rep < 5; rep++) {  // the first launch warms the clocks up; best of the rest
        k_stream<KIND, K><<<1, lanes>>>(1.0 - 0x1p-40, 0x1p-41, 10.0, 2.5625f, kPasses, d_cyc,
                                        d_sink);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(cyc.data(), d_cyc, (lanes / 64) * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost));
        const unsigned long long worst = *std::max_element(cyc.begin(), cyc.begin() + lanes / 64);
        if (rep > 0) best = std::min(best, (double)worst / kPasses);
    }
    *per_pass = best;
    return 0;
}

int main() {
    unsigned long long* d_cyc;
    double* d_sink;
    CHECK(hipMalloc(&d_cyc, (kMaxLanes / 64) * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_sink, kMaxLanes * sizeof(double)));
    const char* names[3] = {"v_cmp_le_f64 |x|, s[..]", "v_cmp_lt_f32 |hi|, s",
                            "v_or3_b32 + v_cmp_lt_f32"};
    printf("16 independent v_fma_f64 per pass, %d passes, slowest wave; clock: s_memtime\n",
           kPasses);
    for (int lanes : {256, 1024}) {
        double base, c2, c4;
        if (run<F64, 0>(lanes, d_cyc, d_sink, &base)) return 1;
        printf("%d wave(s) per SIMD: k = 0 %.1f cycles per pass (%.2f SIMD cycles per FMA)\n",
               lanes / 256, base, base / 16 / (lanes / 256));
        for (int kind = 0; kind < 3; kind++) {
            int rc = kind == F64   ? run<F64, 2>(lanes, d_cyc, d_sink, &c2) |
                                       run<F64, 4>(lanes, d_cyc, d_sink, &c4)
                     : kind == F32 ? run<F32, 2>(lanes, d_cyc, d_sink, &c2) |
                                         run<F32, 4>(lanes, d_cyc, d_sink, &c4)
                                   : run<OR3, 2>(lanes, d_cyc, d_sink, &c2) |
                                         run<OR3, 4>(lanes, d_cyc, d_sink, &c4);
            if (rc) return 1;
            // a wave's clock runs while its SIMD issues for the other waves: / waves = SIMD cycles
            const int waves = lanes / 256;
            printf("  %-26s k = 2 %.1f, k = 4 %.1f cycles per pass: %.2f / %.2f SIMD cycles per "
                   "added %s\n", names[kind], c2, c4, (c2 - base) / 2 / waves,
                   (c4 - base) / 4 / waves, kind == OR3 ? "pair" : "compare");
        }
    }
    (void)hipFree(d_cyc);
    (void)hipFree(d_sink);
    return 0;
}
