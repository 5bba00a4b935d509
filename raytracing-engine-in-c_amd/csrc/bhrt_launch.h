// bhrt_launch.h -- host-side launch geometry shared by the .hip units (geodesic.hip, paths.hip,
// kerr.hip): the current device, its CU count, a kernel's resident workgroups and the grid of a
// grid-stride pass. Everything is in an unnamed namespace, so each unit that includes this has its
// own copy of the CU-count cache: one attribute query per unit and device.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>

namespace {

// Launch geometry is cached per device: a process may drive several devices (bhrt_render_frame
// splits a frame over every visible one) from several host threads. Every cached value is a
// pure function of (device, kernel), so concurrent first calls may both compute it and store
// the same value; the atomics make that race-free without a lock on the launch path.
constexpr int kMaxDev = 64;
std::atomic<int> g_cus[kMaxDev];

inline int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) dev = 0;
    return dev;
}

inline int device_cus(int dev) {
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
inline int resident_blocks(const void* fn, int dev, int lanes = 256) {
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, lanes, 0);
    if (per_cu <= 0) per_cu = 1;
    return device_cus(dev) * per_cu;
}

// resident_blocks of kernel FN on the current device, asked once per kernel and device
template <auto FN>
int resident_blocks_cached(int lanes) {
    static std::atomic<int> cache[kMaxDev];
    const void* const fn = reinterpret_cast<const void*>(FN);
    const int dev = current_device();
    int blocks = cache[dev].load(std::memory_order_relaxed);
    if (blocks == 0) {
        blocks = resident_blocks(fn, dev, lanes);
        cache[dev].store(blocks, std::memory_order_relaxed);
    }
    return blocks;
}

// grid of a grid-stride elementwise kernel over n items (at most one resident wave of blocks)
inline int grid_for(const void* fn, int n) {
    long blocks = ((long)n + 255) / 256;
    const long cap = resident_blocks(fn, current_device());
    if (blocks > cap) blocks = cap;
    return blocks < 1 ? 1 : (int)blocks;
}

}  // namespace
