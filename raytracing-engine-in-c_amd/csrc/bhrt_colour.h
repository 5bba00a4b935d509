// bhrt_colour.h -- the frame colour contract and the sky-map lookup as device functions, shared by
// the kernels of geodesic.hip, paths.hip, frames.hip and checks.hip (through bhrt_trace_core.h,
// which includes this) and of kerr.hip. Included inside the including file's unnamed namespace,
// after `using Scene = bhrt_scene_k;`. The text below was geodesic.hip's own, moved here unchanged:
// every function is the same IEEE operation sequence wherever it is inlined.

__device__ __forceinline__ double clampd(double v, double lo, double hi) {
    if (v < lo) return lo;  // math_util.c:505-509 (NaN passes through)
    if (v > hi) return hi;
    return v;
}

// Frame colour contract, one elementwise pass after the trace:
// calculate_disk_temperature + temperature_to_rgb (+ apply_relativistic_effects) for disk
// hits, black for the horizon, the sky gradient of raytracer.c:1150-1157 otherwise.
// (unsigned char)(std::min(1.0f, v) * 255.0f) as the visualizer's x86 build evaluates it:
// std::min keeps 1.0f for NaN, the cast truncates toward zero and keeps the low byte.
__device__ __forceinline__ unsigned to_u8(float v) {
    const float m = (v < 1.0f) ? v : 1.0f;
    return (unsigned)(int)(m * 255.0f) & 0xffu;
}


// Black for the horizon, the sky gradient of raytracer.c:1150-1157 on the ray direction's y
// otherwise (every ray of a scene without a disk)
__device__ __forceinline__ void colour_sky(int res, double dy, double& r, double& g, double& b) {
#pragma clang fp contract(off)
    if (res == RAY_HORIZON) {
        r = g = b = 0.0;
    } else {
        const double t = 0.5 * (dy + 1.0);
        r = (1.0 - t) * 1.0 + t * 0.5;
        g = (1.0 - t) * 1.0 + t * 0.7;
        b = (1.0 - t) * 1.0 + t * 1.0;
    }
}

// The frame colour contract of one ray: calculate_disk_temperature +
// temperature_to_rgb (+ apply_relativistic_effects with BHRT_FLAG_DOPPLER) of a disk hit at
// (hx, hy), black for the horizon, the sky gradient of raytracer.c:1150-1157 on the ray
// direction's y otherwise. Written by the trace kernel at the ray's exit (colour_fused) or by
// the separate k_colour pass.
__device__ __forceinline__ void colour_of(const Scene& sc, int res, double hx, double hy,
                                          double dx, double dy, double dz, double& r,
                                          double& g, double& b) {
    // no FP contraction here: the colour is then the same IEEE operation sequence wherever it
    // is inlined (the trace kernel's exit or the separate k_colour pass), so both colour paths
    // give the same bits (test_display_path_rgba), as the reference's own non-FMA build does
#pragma clang fp contract(off)
    if (res == RAY_DISK) {
        const double rxy = sqrt(hx * hx + hy * hy);  // raytracer.c:201-228
        double nr = (rxy - sc.disk_in) / (sc.disk_out - sc.disk_in);
        nr = clampd(nr, 0.0, 1.0);
        // pow(1 - nr, 0.75) as sqrt(u) * sqrt(sqrt(u)), u in [0, 1] (a few ulp: the colour
        // contract's tolerance is 1e-5)
        const double su = sqrt(1.0 - nr);
        const double T = clampd(sc.disk_tscale * (2000.0 + 18000.0 * (su * sqrt(su))),
                                1000.0, 40000.0);  // math_util.c:463-503
        const double t = (T - 1000.0) / (40000.0 - 1000.0);
        r = (t < 0.5) ? t * 2.0 : 1.0;
        g = (t < 0.25) ? 0.0 : ((t < 0.75) ? (t - 0.25) * 2.0 : 1.0);
        b = (t < 0.5) ? 0.0 : (t - 0.5) * 2.0;
        const double br = 0.2 + 0.8 * (t * t);
        r *= br;
        g *= br;
        b *= br;
        if (sc.flags & BHRT_FLAG_DOPPLER) {  // raytracer.c:233-294
            // sin, cos of atan2(hy, hx) as hy / rxy, hx / rxy (rxy > 0: a disk hit lies at
            // rxy >= disk_in), pow(dop, 4) as two squarings, dop / (1 / sqrt(f)) as
            // dop * sqrt(f): each within a few ulp of the libm forms
            // (rxy = 0 -- a zero inner radius -- is atan2(+-0, +0) = +-0 or atan2(+-0, -0) =
            // +-pi, whose sin, cos are (+-0, 1) and (+-RN(sin pi), -1): selects, no libm call
            // in the trace kernel)
            const double ir = 1.0 / rxy;
            double sp = hy * ir, cp = hx * ir;
            if (!(rxy > 0.0)) {
                const bool neg_x = __builtin_signbit(hx);
                sp = neg_x ? __builtin_copysign(1.2246467991473532e-16, hy) : hy;
                cp = neg_x ? -1.0 : 1.0;
            }
            const double dop = 1.0 + ((dx * -sp + dy * cp) + dz * 0.0) * 0.5;
            const double z = dop * sqrt(1.0 - sc.rs / rxy);
            if (z < 1.0) {
                b *= z;
                r = fmin(1.0, r * (2.0 - z));
            } else {
                r *= 2.0 - z;
                b = fmin(1.0, b * z);
            }
            const double d2 = dop * dop, beam = d2 * d2;
            r = clampd(r * beam, 0.0, 1.0);
            g = clampd(g * beam, 0.0, 1.0);
            b = clampd(b * beam, 0.0, 1.0);
        }
    } else {
        colour_sky(res, dy, r, g, b);
    }
}

// Sky maps (the rule: include/bhrt_api.h "Sky maps"; tests/sky_rule.py restates it): the
// bilinear lookup of direction d in the launch's equirectangular map. IEEE double, no
// contraction, so the trace kernel's exit, the separate colour pass and k_sky_lookup give the same
// bits. Every index is wrapped (columns) or clamped (rows) after it is formed, so no operand --
// not even a NaN -- reads outside the map's w * h texels.
__device__ __forceinline__ void sky_lookup(const bhrt_sky_k& sk, double dx, double dy, double dz,
                                           double& r, double& g, double& b) {
#pragma clang fp contract(off)
    const double L = sqrt((dx * dx + dy * dy) + dz * dz);
    if (!(L > 0.0 && L <= 1.79769313486231570815e+308)) {  // zero, overflowed or NaN: black
        r = g = b = 0.0;
        return;
    }
    const double th = acos(clampd(dz / L, -1.0, 1.0));
    const double ph = atan2(dy, dx);
    const double fx = (ph + 3.14159265358979323846) * sk.sx - 0.5;
    const double fy = th * sk.sy - 0.5;
    const double fi = floor(fx), fj = floor(fy);
    const double wx = fx - fi, wy = fy - fj;
    const int w = sk.w, h = sk.h;
    int i0 = (int)fi % w, i1 = ((int)fi + 1) % w;
    i0 += i0 < 0 ? w : 0;
    i1 += i1 < 0 ? w : 0;
    const int j0 = min(max((int)fj, 0), h - 1), j1 = min(max((int)fj + 1, 0), h - 1);
    const float4* const T = static_cast<const float4*>(sk.tex);
    const float4 t00 = T[(size_t)j0 * w + i0], t01 = T[(size_t)j0 * w + i1];
    const float4 t10 = T[(size_t)j1 * w + i0], t11 = T[(size_t)j1 * w + i1];
    const double ux = 1.0 - wx, uy = 1.0 - wy;
    r = ((double)t00.x * ux + (double)t01.x * wx) * uy + ((double)t10.x * ux + (double)t11.x * wx) * wy;
    g = ((double)t00.y * ux + (double)t01.y * wx) * uy + ((double)t10.y * ux + (double)t11.y * wx) * wy;
    b = ((double)t00.z * ux + (double)t01.z * wx) * uy + ((double)t10.z * ux + (double)t11.z * wx) * wy;
}

// The colour of one ray of a sky launch: disk and horizon as colour_of; a RAY_MAX_DISTANCE ray
// looks up its exit chord c (a chord with a non-finite component, or whose squared length is not
// > 0, does not count); every other ray the direction the gradient reads, d. `res` is the ray's
// full class. One function for the trace kernel's exit and the separate pass.
// NOT inlined, the one call of the sky instantiations (at a ray's exit, outside the iterations):
// inlined into k_trace, the lookup's acos / atan2 changed how the compiler compiled the ITERATIONS
// around it -- on the few rays per frame that take a rare path (a wide trig shift, the literal
// accelerations) it folded the other product of an a*b + c*d into the FMA -- and a disk pixel of
// a sky frame was not the flagless frame's bit for bit (C2 at max distance 20, 48x27: 5 of 774
// disk pixels, 1.7e-14 relative). Behind a call the iterations compile as the plain
// instantiation's, and the disk and horizon pixels are its bits (test_gpu_sky.py).
template <bool DISK>
__device__ __attribute__((noinline)) void colour_of_sky(const Scene& sc, const bhrt_sky_k& sk, int res,
                                              double hx, double hy, double dx, double dy,
                                              double dz, double cx, double cy, double cz,
                                              double& r, double& g, double& b) {
#pragma clang fp contract(off)
    if (res == RAY_DISK || res == RAY_HORIZON) {
        if constexpr (DISK)
            colour_of(sc, res, hx, hy, dx, dy, dz, r, g, b);
        else
            colour_sky(res, dy, r, g, b);
        return;
    }
    double vx = dx, vy = dy, vz = dz;
    if (res == RAY_MAX_DISTANCE) {
        const double l2 = (cx * cx + cy * cy) + cz * cz;
        const bool fin = fabs(cx) <= 1.79769313486231570815e+308 &&
                         fabs(cy) <= 1.79769313486231570815e+308 &&
                         fabs(cz) <= 1.79769313486231570815e+308;
        if (fin && l2 > 0.0) {
            vx = cx;
            vy = cy;
            vz = cz;
        }
    }
    sky_lookup(sk, vx, vy, vz, r, g, b);
}

__device__ __forceinline__ void store_colour(const bhrt_frame_soa& s, int i, double r, double g,
                                             double b) {
    if (s.rgb_r) {
        s.rgb_r[i] = r;
        s.rgb_g[i] = g;
        s.rgb_b[i] = b;
    }
    if (s.rgba32f || s.rgba8) {  // the display path (renderer.cpp:2090-2125)
        const float fr = (float)r, fg = (float)g, fb = (float)b;
        if (s.rgba32f) reinterpret_cast<float4*>(s.rgba32f)[i] = make_float4(fr, fg, fb, 1.0f);
        if (s.rgba8)
            reinterpret_cast<unsigned*>(s.rgba8)[i] =
                to_u8(fr) | (to_u8(fg) << 8) | (to_u8(fb) << 16) | (to_u8(1.0f) << 24);
    }
}
