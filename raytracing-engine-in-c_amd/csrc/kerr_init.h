/*
 * kerr_init.h -- the initial data of the Kerr-Schild null-ray rule (include/bhrt_api.h "Physical
 * geodesics") as one scalar function, compiled into the kernel (kerr.hip) and into the host
 * (kerr.c: bhrt_kerr_ray_init, and the refusal of an origin without a static observer). One
 * operation per rounding, no contraction, so both give the same bits. The particle rule's step
 * from a coordinate velocity to a momentum ("Physical particles") stands here in the same way
 * (kerr.hip k_kerr_particles; kerr.c bhrt_kerr_particle_state).
 */
#ifndef BHRT_KERR_INIT_H
#define BHRT_KERR_INIT_H

#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#define BHRT_KERR_HD __host__ __device__ __forceinline__
#else
#define BHRT_KERR_HD static inline
#endif

/* n = d / |d|, |d| = sqrt((dx^2 + dy^2) + dz^2) */
BHRT_KERR_HD void bhrt_kerr_unit(const double d[3], double n[3]) {
#ifdef __HIPCC__
#pragma clang fp contract(off)
#endif
    const double L = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    n[0] = d[0] / L;
    n[1] = d[1] / L;
    n[2] = d[2] / L;
}

/* f, r and l at (x, y, z) for spin a (a2 = a^2) and two_m = 2 M, in the rule's order. Returns 1
 * where a static observer exists there: f < 1 and r > r_plus (a NaN fails both). */
BHRT_KERR_HD int bhrt_kerr_origin(double x, double y, double z, double a, double a2, double two_m,
                                  double r_plus, double* f_out, double l[3]) {
#ifdef __HIPCC__
#pragma clang fp contract(off)
#endif
    const double z2 = z * z;
    const double rho2 = (x * x + y * y) + z2;
    const double w = rho2 - a2;
    const double D = sqrt(w * w + 4.0 * a2 * z2);
    const double r2 = (w + D) / 2.0;
    const double r = sqrt(r2);
    const double G = r2 * r2 + a2 * z2;
    const double S = r2 + a2;
    const double f = two_m * (r * r2) / G;
    l[0] = (r * x + a * y) / S;
    l[1] = (r * y - a * x) / S;
    l[2] = z / r;
    *f_out = f;
    return f < 1.0 && r > r_plus;
}

/* p and E of the static observer's photon of local energy 1 along unit n, from f and l there */
BHRT_KERR_HD void bhrt_kerr_photon(double f, const double l[3], const double n[3], double p[3],
                                   double* E) {
#ifdef __HIPCC__
#pragma clang fp contract(off)
#endif
    const double kappa = sqrt(1.0 - f);
    const double ln = (l[0] * n[0] + l[1] * n[1]) + l[2] * n[2];
    const double s = (kappa - 1.0) * ln;
    const double v0 = n[0] + s * l[0], v1 = n[1] + s * l[1], v2 = n[2] + s * l[2];
    const double lv = (l[0] * v0 + l[1] * v1) + l[2] * v2;
    const double kt = 1.0 / kappa + f * lv / (1.0 - f);
    const double c = f * (kt + lv);
    p[0] = v0 + c * l[0];
    p[1] = v1 + c * l[1];
    p[2] = v2 + c * l[2];
    *E = kappa;
}

/* f and l at (x, y, z) as bhrt_kerr_origin forms them, with no test; returns r */
BHRT_KERR_HD double bhrt_kerr_fields(double x, double y, double z, double a, double a2, double two_m,
                                     double* f_out, double l[3]) {
#ifdef __HIPCC__
#pragma clang fp contract(off)
#endif
    const double z2 = z * z;
    const double rho2 = (x * x + y * y) + z2;
    const double w = rho2 - a2;
    const double D = sqrt(w * w + 4.0 * a2 * z2);
    const double r2 = (w + D) / 2.0;
    const double r = sqrt(r2);
    const double G = r2 * r2 + a2 * z2;
    const double S = r2 + a2;
    *f_out = two_m * (r * r2) / G;
    l[0] = (r * x + a * y) / S;
    l[1] = (r * y - a * x) / S;
    l[2] = z / r;
    return r;
}

/* The particle rule's "From velocity to momentum": p, E and u^t of the unit-mass particle with
 * coordinate velocity v = dx/dt, from f and l at its position. Returns 1 where v is timelike there
 * (N finite and > 0), else 0 with nothing written. */
BHRT_KERR_HD int bhrt_kerr_particle(double f, const double l[3], const double v[3], double p[3],
                                    double* E, double* ut) {
#ifdef __HIPCC__
#pragma clang fp contract(off)
#endif
    const double w = 1.0 + ((l[0] * v[0] + l[1] * v[1]) + l[2] * v[2]);
    const double N = (1.0 - ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])) - f * (w * w);
    if (!(N > 0.0 && N <= DBL_MAX)) return 0;
    const double u = 1.0 / sqrt(N);
    const double c = f * w;
    p[0] = u * (v[0] + c * l[0]);
    p[1] = u * (v[1] + c * l[1]);
    p[2] = u * (v[2] + c * l[2]);
    *E = u * (1.0 - c);
    *ut = u;
    return 1;
}

#endif
