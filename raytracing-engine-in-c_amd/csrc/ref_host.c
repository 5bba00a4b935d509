/*
 * ref_host.c -- the reference's host functions that a drop-in caller links against, restated:
 * the vector3D_* helpers and clamp (math_util.c), and the scalar functions of the ray path
 * (raytracer.c, spacetime.c, math_util.c). Plain C over libm: no HIP, no state. Built without FP
 * contraction; tests/test_abi.py pins every one bit for bit.
 */
#include <math.h>
#include <stdlib.h>

#pragma GCC visibility push(default)
#include "../../include/bhrt_api.h"
#pragma GCC visibility pop

/* ======================================================================================= */
/* host vector helpers (math_util.c:31-122 semantics; also the drop-in vector3D_* symbols)  */
/* ======================================================================================= */
Vector3D vector3D_add(const Vector3D a, const Vector3D b) {
    Vector3D r = {a.x + b.x, a.y + b.y, a.z + b.z};
    return r;
}
Vector3D vector3D_sub(const Vector3D a, const Vector3D b) {
    Vector3D r = {a.x - b.x, a.y - b.y, a.z - b.z};
    return r;
}
Vector3D vector3D_scale(const Vector3D v, double s) {
    Vector3D r = {v.x * s, v.y * s, v.z * s};
    return r;
}
double vector3D_dot(const Vector3D a, const Vector3D b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
Vector3D vector3D_cross(const Vector3D a, const Vector3D b) {
    Vector3D r = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
    return r;
}
double vector3D_length(const Vector3D v) { return sqrt(vector3D_dot(v, v)); }
Vector3D vector3D_normalize(const Vector3D v) {
    double l = vector3D_length(v);
    if (l < BH_EPSILON) {
        Vector3D z = {0.0, 0.0, 0.0};
        return z;
    }
    return vector3D_scale(v, 1.0 / l);
}
double clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* ======================================================================================= */
/* scalar helpers of the ray path (host side of the drop-in)                                */
/* ======================================================================================= */
int check_disk_intersection(const Vector3D* p, const Vector3D* v, const Vector3D* n,
                            const AccretionDiskParams* disk, Vector3D* q) {
    double den = vector3D_dot(*v, *n);
    if (fabs(den) < BH_EPSILON) return 0;
    double t = -(vector3D_dot(*p, *n)) / den;
    if (t < 0.0) return 0;
    *q = vector3D_add(*p, vector3D_scale(*v, t));
    double r = sqrt(q->x * q->x + q->y * q->y);
    return r >= disk->inner_radius && r <= disk->outer_radius;
}

void temperature_to_rgb(double T, double rgb[3]) {
    T = clamp(T, 1000.0, 40000.0);
    double t = (T - 1000.0) / (40000.0 - 1000.0);
    rgb[0] = t < 0.5 ? t * 2.0 : 1.0;
    rgb[1] = t < 0.25 ? 0.0 : (t < 0.75 ? (t - 0.25) * 2.0 : 1.0);
    rgb[2] = t < 0.5 ? 0.0 : (t - 0.5) * 2.0;
    double br = 0.2 + 0.8 * (t * t);
    rgb[0] *= br;
    rgb[1] *= br;
    rgb[2] *= br;
}

void calculate_disk_temperature(const Vector3D* p, const BlackHoleParams* bh,
                                const AccretionDiskParams* disk, double* T, double color[3]) {
    (void)bh;
    double r = sqrt(p->x * p->x + p->y * p->y);
    double nr = clamp((r - disk->inner_radius) / (disk->outer_radius - disk->inner_radius), 0.0, 1.0);
    *T = disk->temperature_scale * (2000.0 + 18000.0 * pow(1.0 - nr, 0.75));
    temperature_to_rgb(*T, color);
}

double calculate_time_dilation(double r, const BlackHoleParams* bh) {
    return 1.0 / sqrt(1.0 - bh->schwarzschild_radius / r);
}

void apply_relativistic_effects(const Vector3D* p, const Vector3D* v, const BlackHoleParams* bh,
                                double c[3], double* dop_out) {
    double r = sqrt(p->x * p->x + p->y * p->y);
    double phi = atan2(p->y, p->x);
    Vector3D tangent = {-sin(phi), cos(phi), 0.0};
    double dop = 1.0 + vector3D_dot(*v, tangent) * 0.5;
    double z = dop / calculate_time_dilation(r, bh);
    if (z < 1.0) {
        c[2] *= z;
        c[0] = fmin(1.0, c[0] * (2.0 - z));
    } else {
        c[0] *= 2.0 - z;
        c[2] = fmin(1.0, c[2] * z);
    }
    double beam = pow(dop, 4);
    c[0] = clamp(c[0] * beam, 0.0, 1.0);
    c[1] = clamp(c[1] * beam, 0.0, 1.0);
    c[2] = clamp(c[2] * beam, 0.0, 1.0);
    if (dop_out) *dop_out = dop;
}

void generate_gpu_shader_params(const BlackHoleParams* bh, const AccretionDiskParams* dk,
                                double observer_distance, double fov, GPUShaderParams* p) {
    if (!bh || !p) return;
    p->mass = bh->mass;
    p->spin = bh->spin;
    p->schwarzschild_radius = 2.0 * bh->mass;
    p->observer_distance = observer_distance;
    p->fov = fov;
    if (dk) {
        p->disk_inner_radius = dk->inner_radius;
        p->disk_outer_radius = dk->outer_radius;
        p->disk_temp_scale = dk->temperature_scale;
    } else {
        p->disk_inner_radius = 3.0 * p->schwarzschild_radius;
        p->disk_outer_radius = 20.0 * p->schwarzschild_radius;
        p->disk_temp_scale = 1.0;
    }
}

double halton_sequence(int index, int base) {
    double result = 0.0, f = 1.0;
    for (; index > 0; index /= base) {
        f /= base;
        result += f * (index % base);
    }
    return result;
}

SchwarzschildMetric calculate_schwarzschild_metric(double r, const BlackHoleParams* bh) {
    SchwarzschildMetric m;
    double rs = bh->schwarzschild_radius;
    if (r <= rs + BH_EPSILON) r = rs + BH_EPSILON;
    m.g_tt = -(1.0 - rs / r);
    m.g_rr = 1.0 / (1.0 - rs / r);
    m.g_thth = r * r;
    m.g_phph = r * r; /* r*r*sin^2(pi/2), sin(pi/2) == 1.0 in double */
    return m;
}

void cartesian_to_spherical(const Vector3D* c, Vector3D* s) {
    double r = sqrt(c->x * c->x + c->y * c->y + c->z * c->z);
    double th = r > BH_EPSILON ? acos(c->z / r) : 0.0;
    double ph = atan2(c->y, c->x);
    if (ph < 0.0) ph += BH_TWO_PI;
    s->x = r;
    s->y = th;
    s->z = ph;
}

void spherical_to_cartesian(const Vector3D* s, Vector3D* c) {
    c->x = s->x * sin(s->y) * cos(s->z);
    c->y = s->x * sin(s->y) * sin(s->z);
    c->z = s->x * cos(s->y);
}

double get_isco_radius(const BlackHoleParams* bh) {
    double M = bh->mass, a = bh->spin * M;
    if (bh->spin == 0.0) return 6.0 * M;
    double third = 1.0 / 3.0;
    double z1 = 1.0 + pow(1.0 - a * a / (M * M), third) *
                          (pow(1.0 + a / (M), third) + pow(1.0 - a / (M), third));
    double z2 = sqrt(3.0 * a * a / (M * M) + z1 * z1);
    return M * (3.0 + z2 - sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2)));
}

void initialize_black_hole_params(BlackHoleParams* bh, double mass, double spin, double charge) {
    bh->mass = mass;
    bh->spin = spin;
    bh->charge = charge;
    bh->schwarzschild_radius = 2.0 * mass; /* every branch: spacetime.c:338,348,358 */
    bh->ergosphere_radius = 2.0 * mass;
    if (spin == 0.0 && charge == 0.0) {
        bh->r_plus = 2.0 * mass;
        bh->r_minus = 0.0;
    } else {
        double a = spin * mass;
        double q2 = (spin > 0.0 && charge == 0.0) ? 0.0 : charge * charge;
        double s = q2 == 0.0 ? sqrt(mass * mass - a * a) : sqrt(mass * mass - a * a - q2);
        bh->r_plus = mass + s;
        bh->r_minus = mass - s;
    }
    bh->isco_radius = get_isco_radius(bh);
}

/* ---- generic host integrators (math_util.c:162-457; debug printing not reproduced) ---- */
void rk4_integrate(ODEFunction f, double* y, int n, double t, double h, void* params) {
    double* w = (double*)malloc(sizeof(double) * 5 * (size_t)(n > 0 ? n : 1));
    if (!w) return;
    double *k1 = w, *k2 = w + n, *k3 = w + 2 * n, *k4 = w + 3 * n, *yt = w + 4 * n;
    f(t, y, k1, params);
    for (int i = 0; i < n; i++) yt[i] = y[i] + 0.5 * h * k1[i];
    f(t + 0.5 * h, yt, k2, params);
    for (int i = 0; i < n; i++) yt[i] = y[i] + 0.5 * h * k2[i];
    f(t + 0.5 * h, yt, k3, params);
    for (int i = 0; i < n; i++) yt[i] = y[i] + h * k3[i];
    f(t + h, yt, k4, params);
    for (int i = 0; i < n; i++) y[i] += h * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) / 6.0;
    free(w);
}

int rkf45_integrate(ODEFunction f, double y[], int n, double* t, double h, double* h_next,
                    double eps_rel, void* params) {
    static const double A[6] = {0.0, 1.0 / 4.0, 3.0 / 8.0, 12.0 / 13.0, 1.0, 1.0 / 2.0};
    static const double B[6][5] = {
        {0, 0, 0, 0, 0},
        {1.0 / 4.0, 0, 0, 0, 0},
        {3.0 / 32.0, 9.0 / 32.0, 0, 0, 0},
        {1932.0 / 2197.0, -7200.0 / 2197.0, 7296.0 / 2197.0, 0, 0},
        {439.0 / 216.0, -8.0, 3680.0 / 513.0, -845.0 / 4104.0, 0},
        {-8.0 / 27.0, 2.0, -3544.0 / 2565.0, 1859.0 / 4104.0, -11.0 / 40.0}};
    static const double C4[6] = {25.0 / 216.0, 0, 1408.0 / 2565.0, 2197.0 / 4104.0, -1.0 / 5.0, 0};
    static const double C5[6] = {16.0 / 135.0, 0, 6656.0 / 12825.0, 28561.0 / 56430.0,
                                 -9.0 / 50.0, 2.0 / 55.0};
    double* w = (double*)malloc(sizeof(double) * 9 * (size_t)(n > 0 ? n : 1));
    if (!w) return 1;
    double* k[6];
    for (int s = 0; s < 6; s++) k[s] = w + s * n;
    double *yt = w + 6 * n, *y4 = w + 7 * n, *y5 = w + 8 * n;
    int rc = 1;
    f(*t, y, k[0], params);
    for (int i = 0; i < n; i++)
        if (isnan(k[0][i]) || isinf(k[0][i])) goto out;
    for (int s = 1; s < 6; s++) {
        for (int i = 0; i < n; i++) {
            /* same left-to-right sums as the unrolled reference: h*b21*k1 for stage 2,
             * h*(b31*k1 + b32*k2 + ...) afterwards */
            double acc;
            if (s == 1) {
                yt[i] = y[i] + h * B[1][0] * k[0][i];
                continue;
            }
            acc = B[s][0] * k[0][i];
            for (int j = 1; j < s; j++) acc = acc + B[s][j] * k[j][i];
            yt[i] = y[i] + h * acc;
        }
        f(*t + h * A[s], yt, k[s], params);
    }
    double max_error = 0.0;
    for (int i = 0; i < n; i++) {
        y4[i] = y[i] + h * (C4[0] * k[0][i] + C4[2] * k[2][i] + C4[3] * k[3][i] + C4[4] * k[4][i]);
        y5[i] = y[i] + h * (C5[0] * k[0][i] + C5[2] * k[2][i] + C5[3] * k[3][i] +
                            C5[4] * k[4][i] + C5[5] * k[5][i]);
        double scale = fmax(fabs(y[i]), fabs(y5[i]));
        if (scale < BH_EPSILON) scale = BH_EPSILON;
        max_error = fmax(max_error, fabs(y5[i] - y4[i]) / scale);
    }
    double ratio = max_error / eps_rel;
    if (ratio <= 1.0) {
        double scale = ratio == 0.0 ? 10.0 : fmax(0.2, fmin(10.0, 0.9 * pow(ratio, -0.2)));
        for (int i = 0; i < n; i++) y[i] = y5[i];
        *t = *t + h;
        *h_next = h * scale;
        rc = 0;
    } else {
        *h_next = h * fmax(0.2, fmin(10.0, 0.9 * pow(ratio, -0.25)));
    }
out:
    free(w);
    return rc;
}
