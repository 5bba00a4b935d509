// paths.hip -- the recorded-path kernels of the geodesic ray tracer: k_path (one ray's path,
// bhrt_launch_path) and k_paths (batched polylines, bhrt_launch_paths), with their launchers. Every
// point is an iteration of bhrt_trace_core.h's ray_iterate in its general, always-select
// instantiation. The host side is paths.c.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bhrt_kernel.h"
#include "bhrt_launch.h"

#pragma clang fp contract(fast)

namespace {

#include "bhrt_trace_core.h"

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
