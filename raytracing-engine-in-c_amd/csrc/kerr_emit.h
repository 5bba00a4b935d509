/*
 * kerr_emit.h -- the redshift of a disk crossing (include/bhrt_api.h "Kerr disk emission") as one
 * scalar function, compiled into the kernel (kerr.hip k_kerr_emit) and into the host
 * (kerr_emit.c: bhrt_kerr_disk_redshift). One operation per rounding, no contraction, so both give
 * the same bits for the same operands.
 */
#ifndef BHRT_KERR_EMIT_H
#define BHRT_KERR_EMIT_H

#include <math.h>

#include "kerr_init.h"

/* g = E_obs / E_emit of a photon with constants E and lz = x p_y - y p_x (of the integrated,
 * time-reversed ray) that meets the equatorial circular orbit of Boyer-Lindquist radius r about a
 * hole of mass M and physical spin a = spin * mass (a2 = a^2), the disk turning about +z in +phi:
 *   Omega = sqrt(M) / (r sqrt(r) + a sqrt(M)),
 *   N = (1 - (2M / r)(1 - a Omega)^2) - Omega^2 (r^2 + a^2),   g = sqrt(N) / (E + Omega lz).
 * 0 where N > 0 or E + Omega lz > 0 fails, or where g is not finite: no circular orbit there. */
BHRT_KERR_HD double bhrt_kerr_emit_g(double r, double a, double a2, double M, double E, double lz) {
#ifdef __HIPCC__
#pragma clang fp contract(off)
#endif
    const double sm = sqrt(M);
    const double om = sm / (r * sqrt(r) + a * sm);
    const double t = 1.0 - a * om;
    const double N = (1.0 - (2.0 * M / r) * (t * t)) - (om * om) * (r * r + a2);
    const double den = E + om * lz;
    const double g = sqrt(N) / den;
    if (!(N > 0.0) || !(den > 0.0) || !(fabs(g) <= 1.79769313486231570815e+308)) return 0.0;
    return g;
}

#endif
