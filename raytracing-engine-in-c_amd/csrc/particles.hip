// particles.hip -- update_particles (src/particle_sim.c:505-566) as a HIP kernel: one lane per
// particle, `steps` updates in registers per launch.
//
// The arithmetic is the reference's, operation for operation and in its evaluation order,
// without FP contraction (the reference's x86-64 build has none): the Euler step of the
// geodesic update (particle_sim.c:232-304) with geodesic_equation's full 4x4x4 Christoffel
// contraction (spacetime.c:95-187, zero entries included, so Inf/NaN velocities propagate as
// they do there), and the Newtonian update (particle_sim.c:306-337). sin/cos/acos/atan2 are
// OCML's (within an ulp or two of glibc).
#include <hip/hip_runtime.h>

#include "bhrt_kernel.h"

#pragma clang fp contract(off)

namespace {

constexpr double kEps = 1.0e-10;                   // BH_EPSILON (math_util.h:21)
constexpr double kTwoPi = 6.28318530717958647692;  // BH_TWO_PI (math_util.h:26-27)

__device__ __forceinline__ double length3(const Vector3D& v) {
    return sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);  // vector3D_length (math_util.c:85-113)
}

// calculate_christoffel_symbols (spacetime.c:95-161) then geodesic_equation (:166-187)
__device__ __forceinline__ void geodesic_accel(double r, double theta, const double v[4],
                                               const bhrt_particle_k& k, double acc[4]) {
    double G[4][4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int l = 0; l < 4; l++) G[i][j][l] = 0.0;
    if (k.spin0) {
        const double rs = k.rs;
        if (r <= rs + kEps) r = rs + kEps;
        const double st = sin(theta), ct = cos(theta);
        G[0][0][1] = G[0][1][0] = rs / (2.0 * r * (r - rs));
        G[1][0][0] = rs * (r - rs) / (2.0 * r * r * r);
        G[1][1][1] = -rs / (2.0 * r * (r - rs));
        G[1][2][2] = -(r - rs);
        G[1][3][3] = -(r - rs) * st * st;
        G[2][1][2] = G[2][2][1] = 1.0 / r;
        G[2][3][3] = -st * ct;
        G[3][1][3] = G[3][3][1] = 1.0 / r;
        G[3][2][3] = G[3][3][2] = ct / st;
    } else {  // the reference's Kerr subset (:126-158)
        const double M = k.M, a = k.a;
        if (r <= k.r_plus + kEps) r = k.r_plus + kEps;
        const double st = sin(theta), ct = cos(theta);
        const double st2 = st * st, ct2 = ct * ct;
        const double Sigma = r * r + a * a * ct2;
        const double Sigma_sq = Sigma * Sigma;
        G[0][0][1] = M * (r * r - a * a * ct2) / Sigma_sq;
        G[0][1][0] = G[0][0][1];
        G[0][1][3] = -a * M * st2 * (r * r - a * a * ct2) / Sigma_sq;
        G[0][3][1] = G[0][1][3];
    }
#pragma unroll
    for (int mu = 0; mu < 4; mu++) {
        double s = 0.0;
#pragma unroll
        for (int al = 0; al < 4; al++)
#pragma unroll
            for (int be = 0; be < 4; be++) s -= G[mu][al][be] * v[al] * v[be];
        acc[mu] = s;
    }
}

// update_particle_geodesic (particle_sim.c:232-304)
__device__ __forceinline__ void step_geodesic(Particle& p, const bhrt_particle_k& k) {
    const double x = p.position.x, y = p.position.y, z = p.position.z;
    const double r = sqrt(x * x + y * y + z * z);  // cartesian_to_spherical (spacetime.c:201-224)
    double theta = 0.0;
    if (r > kEps) theta = acos(z / r);
    double phi = atan2(y, x);
    if (phi < 0.0) phi += kTwoPi;
    double st[8] = {0.0, r, theta, phi, 1.0, 0.0, 0.0, 0.0};
    const double v_mag = length3(p.velocity);
    st[5] = v_mag * cos(theta) * cos(phi);
    st[6] = v_mag * sin(phi);
    st[7] = v_mag * sin(theta) * cos(phi);
    double acc[4];
    const double vel[4] = {st[4], st[5], st[6], st[7]};
    geodesic_accel(st[1], st[2], vel, k, acc);
    const double d[8] = {st[4], st[5], st[6], st[7], acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] += d[i] * k.dt;
    p.position.x = st[1] * sin(st[2]) * cos(st[3]);  // spherical_to_cartesian (spacetime.c:229)
    p.position.y = st[1] * sin(st[2]) * sin(st[3]);
    p.position.z = st[1] * cos(st[2]);
    const double v_r = st[5], v_theta = st[6], v_phi = st[7];
    const double s_t = sin(theta), c_t = cos(theta), s_p = sin(phi), c_p = cos(phi);
    p.velocity.x = v_r * s_t * c_p + r * v_theta * c_t * c_p - r * s_t * v_phi * s_p;
    p.velocity.y = v_r * s_t * s_p + r * v_theta * c_t * s_p + r * s_t * v_phi * c_p;
    p.velocity.z = v_r * c_t - r * v_theta * s_t;
    p.time_dilation = 1.0 / sqrt(1.0 - k.rs / st[1]);  // calculate_time_dilation (:192-196)
}

// update_particle_newtonian (particle_sim.c:306-337)
__device__ __forceinline__ void step_newtonian(Particle& p, const bhrt_particle_k& k) {
    const double r = length3(p.position);
    const double accel_mag = k.M / (r * r);
    const double inv = -1.0 / r;
    const double ax = p.position.x * inv * accel_mag, ay = p.position.y * inv * accel_mag,
                 az = p.position.z * inv * accel_mag;
    p.velocity.x = p.velocity.x + ax * k.dt;
    p.velocity.y = p.velocity.y + ay * k.dt;
    p.velocity.z = p.velocity.z + az * k.dt;
    p.position.x = p.position.x + p.velocity.x * k.dt;
    p.position.y = p.position.y + p.velocity.y * k.dt;
    p.position.z = p.position.z + p.velocity.z * k.dt;
}

// update_particles body (:519-562) for particle i: `steps` updates in registers; the active flag after
__device__ __forceinline__ int update_one(Particle* ps, int i, const bhrt_particle_k& k, int steps) {
    Particle p = ps[i];
    const double rs20 = 20.0 * k.rs;
    for (int s = 0; s < steps && p.active; s++) {
        p.age += k.dt;
        const double r = length3(p.position);
        if (p.type == PARTICLE_TEST && r < rs20)
            step_geodesic(p, k);
        else
            step_newtonian(p, k);
        if (length3(p.position) <= k.rs) p.active = 0;
    }
    ps[i] = p;
    return p.active;
}

// the workgroup's count of set flags into block_active[blockIdx.x]: a ballot per wave, the four
// waves' counts summed through LDS. Every lane of the workgroup calls it (a barrier inside). In
// the update kernel it costs nothing that HIP events can see (profiles/particles_resident).
__device__ __forceinline__ void block_count(bool active, int* block_active) {
    __shared__ int wave_count[4];
    const unsigned long long m = __ballot(active);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0)
        block_active[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

// COUNT = false: the kernel of update_particles and bhrt_update_particles_steps. COUNT = true
// (device-resident systems, particles_resident.c): the same arithmetic, and the workgroup's number
// of particles active AFTER the update into block_active[blockIdx.x]; lanes past count add 0 and
// stay for the barrier.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_update_particles(Particle* ps, int count,
                                                          const bhrt_particle_k k, int steps,
                                                          int* block_active) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!COUNT) {
        if (i >= count) return;
        (void)update_one(ps, i, k, steps);
    } else {
        int active = 0;
        if (i < count) active = update_one(ps, i, k, steps);
        block_count(active != 0, block_active);
    }
}

// block_active[] of an array as it stands (after an upload): the flags alone are read
__global__ __launch_bounds__(256) void k_particles_count(const Particle* ps, int count,
                                                         int* block_active) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    block_count(i < count && ps[i].active != 0, block_active);
}

// Exclusive scan of block_active[0, nblocks) into offsets[0, nblocks], offsets[nblocks] = the
// total. ONE workgroup walks the array in chunks of 256 x kScanItems with a running carry: no
// workgroup waits for another, whatever the size.
constexpr int kScanItems = 16;
__global__ __launch_bounds__(256) void k_particles_scan(const int* block_active, int nblocks,
                                                        int* offsets) {
    __shared__ int wave_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nblocks; base += 256 * kScanItems) {
        const int first = base + (int)threadIdx.x * kScanItems;
        int v[kScanItems];
        int mine = 0;
#pragma unroll
        for (int j = 0; j < kScanItems; j++) {
            v[j] = first + j < nblocks ? block_active[first + j] : 0;
            mine += v[j];
        }
        int incl = mine;  // inclusive scan of the lanes' sums within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; w++) before += wave_sum[w];
        const int chunk = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
        __syncthreads();  // wave_sum is rewritten by the next chunk
        int run = before + (incl - mine);
#pragma unroll
        for (int j = 0; j < kScanItems; j++) {
            if (first + j < nblocks) offsets[first + j] = run;
            run += v[j];
        }
        carry += chunk;
    }
    if (threadIdx.x == 0) offsets[nblocks] = carry;
}

// bh_get_particle_data on the device: the active particle of rank r < max_count (its number among
// the active ones in array order) writes element r of every output. The rank is the workgroup's
// scanned offset + the set flags of the lower waves (LDS) + those of the lower lanes (ballot), so
// no atomic decides a place and a wave's stores are contiguous runs. Elements at or beyond the
// count are not written.
__global__ __launch_bounds__(256) void k_particles_scatter(const Particle* ps, int count,
                                                           const int* offsets, int nblocks,
                                                           int max_count,
                                                           const bhrt_particle_data out) {
    __shared__ int wave_count[4];
    const int base = offsets[blockIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0 && out.count) {
        const int total = offsets[nblocks];
        out.count[0] = total < max_count ? total : max_count;
    }
    // uniform per workgroup, before the barrier: nothing of this workgroup lands
    if (base >= max_count || offsets[blockIdx.x + 1] == base) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool active = i < count && ps[i].active != 0;
    const unsigned long long m = __ballot(active);
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int rank = base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += wave_count[w];
    if (!active || rank >= max_count) return;
    const Particle* p = ps + i;
    const size_t r = (size_t)rank, r3 = 3 * (size_t)rank;
    const Vector3D x = p->position, v = p->velocity;
    if (out.positions) {
        out.positions[r3 + 0] = x.x;
        out.positions[r3 + 1] = x.y;
        out.positions[r3 + 2] = x.z;
    }
    if (out.velocities) {
        out.velocities[r3 + 0] = v.x;
        out.velocities[r3 + 1] = v.y;
        out.velocities[r3 + 2] = v.z;
    }
    if (out.types) out.types[r] = (int32_t)p->type;
    if (out.ids) out.ids[r] = (int32_t)p->id;
    if (out.xyz32) {
        out.xyz32[r3 + 0] = (float)x.x;
        out.xyz32[r3 + 1] = (float)x.y;
        out.xyz32[r3 + 2] = (float)x.z;
    }
    if (out.vel32) {
        out.vel32[r3 + 0] = (float)v.x;
        out.vel32[r3 + 1] = (float)v.y;
        out.vel32[r3 + 2] = (float)v.z;
    }
}

}  // namespace

extern "C" int bhrt_launch_particles(Particle* d, int count, const bhrt_particle_k* k, int steps,
                                     void* stream, void* ev0, void* ev1) {
    hipStream_t st = (hipStream_t)stream;
    if (ev0) (void)hipEventRecord((hipEvent_t)ev0, st);
    if (count > 0 && steps > 0)
        k_update_particles<false><<<(count + 255) / 256, 256, 0, st>>>(d, count, *k, steps, nullptr);
    if (ev1) (void)hipEventRecord((hipEvent_t)ev1, st);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_particles_counted(Particle* d, int count, const bhrt_particle_k* k,
                                             int steps, int* d_block_active, void* stream,
                                             void* ev0, void* ev1) {
    hipStream_t st = (hipStream_t)stream;
    if (ev0) (void)hipEventRecord((hipEvent_t)ev0, st);
    if (count > 0 && steps > 0)
        k_update_particles<true><<<(count + 255) / 256, 256, 0, st>>>(d, count, *k, steps,
                                                                      d_block_active);
    if (ev1) (void)hipEventRecord((hipEvent_t)ev1, st);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_particles_count(const Particle* d, int count, int* d_block_active,
                                           void* stream) {
    if (count > 0)
        k_particles_count<<<(count + 255) / 256, 256, 0, (hipStream_t)stream>>>(d, count,
                                                                                d_block_active);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_particles_scan(const int* d_block_active, int nblocks, int* d_offsets,
                                          void* stream, void* ev0, void* ev1) {
    hipStream_t st = (hipStream_t)stream;
    if (ev0) (void)hipEventRecord((hipEvent_t)ev0, st);
    if (nblocks > 0) k_particles_scan<<<1, 256, 0, st>>>(d_block_active, nblocks, d_offsets);
    if (ev1) (void)hipEventRecord((hipEvent_t)ev1, st);
    return (int)hipGetLastError();
}

extern "C" int bhrt_launch_particles_scatter(const Particle* d, int count, const int* d_offsets,
                                             int max_count, const bhrt_particle_data* out,
                                             void* stream, void* ev0, void* ev1) {
    hipStream_t st = (hipStream_t)stream;
    const int nblocks = (count + 255) / 256;
    if (ev0) (void)hipEventRecord((hipEvent_t)ev0, st);
    if (count > 0)
        k_particles_scatter<<<nblocks, 256, 0, st>>>(d, count, d_offsets, nblocks, max_count, *out);
    if (ev1) (void)hipEventRecord((hipEvent_t)ev1, st);
    return (int)hipGetLastError();
}
