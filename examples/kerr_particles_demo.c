/*
 * kerr_particles_demo.c -- particles that actually orbit, from a plain C caller of libbhrt.so: a
 * ring of circular orbits seeded with bhrt_kerr_orbit_velocity and one plunger, advanced along
 * timelike geodesics of a spin-0.9 Kerr hole by bhrt_particles_kerr_update_device on a
 * device-resident system.
 *
 *   gcc -std=c99 -Iinclude examples/kerr_particles_demo.c -Lraytracing-engine-in-c_amd -lbhrt \
 *       -Wl,-rpath,$PWD/raytracing-engine-in-c_amd -lm -o kerr_particles_demo && ./kerr_particles_demo
 *
 * Every 20 ticks of 0.5 M it prints t, the Boyer-Lindquist radius r(t) of the first three ring
 * particles and of the plunger, and the plunger's E and proper time: the ring radii stay put, the
 * plunger falls from rest at 10 M and is captured at r+ with finite fields.
 */
#include <math.h>
#include <stdio.h>

#include "blackhole_api.h"

enum { RING = 8, N = RING + 1, TICKS = 200, EVERY = 20 };

static double bl_radius(const Vector3D* x, double a) {
    const double w = x->x * x->x + x->y * x->y + x->z * x->z - a * a;
    return sqrt(0.5 * (w + sqrt(w * w + 4.0 * a * a * x->z * x->z)));
}

int main(void) {
    BlackHoleParams bh;
    initialize_black_hole_params(&bh, 1.0, 0.9, 0.0);
    const double a = bh.spin * bh.mass;
    SimulationConfig cfg = {0};
    cfg.time_step = 0.5;

    ParticleSystem sys;
    if (particle_system_init(&sys, N) != 0) return 1;
    for (int i = 0; i < RING; i++) { /* prograde circular orbits at r = 3 M ... 10 M */
        const double r = 3.0 + i, rho = sqrt(r * r + a * a), phi = 0.7 * i;
        const Vector3D pos = {rho * cos(phi), rho * sin(phi), 0.0};
        Vector3D vel;
        if (bhrt_kerr_orbit_velocity(&bh, &pos, 1, &vel) != 0) {
            fprintf(stderr, "no circular orbit at r = %g: %s\n", r, bhrt_last_error());
            return 1;
        }
        add_particle(&sys, &pos, &vel, 1.0, PARTICLE_DISK);
    }
    const Vector3D rest = {0.0, 0.0, 0.0}, far = {10.0, 0.0, 0.5};
    add_particle(&sys, &far, &rest, 1.0, PARTICLE_TEST); /* the plunger */

    bhrt_particles* ps = NULL;
    if (bhrt_particles_create(&sys, &ps) != 0) {
        fprintf(stderr, "bhrt_particles_create: %s\n", bhrt_last_error());
        return 1;
    }
    const bhrt_kerr_particles_params par = {1};
    printf("      t    r[0]      r[1]      r[2]      r[plunger]  E[plunger]  tau[plunger]  active\n");
    for (int t = 0; t <= TICKS; t += EVERY) {
        if (t > 0 && bhrt_particles_kerr_update_device(ps, &bh, &cfg, EVERY, &par, NULL, NULL) != 0) {
            fprintf(stderr, "bhrt_particles_kerr_update_device: %s\n", bhrt_last_error());
            return 1;
        }
        if (bhrt_particles_download(ps, &sys) != 0) {
            fprintf(stderr, "bhrt_particles_download: %s\n", bhrt_last_error());
            return 1;
        }
        const Particle* p = sys.particles;
        printf("%7.1f  %.6f  %.6f  %.6f  %10.6f  %10.6f  %12.6f  %d\n", t * cfg.time_step,
               bl_radius(&p[0].position, a), bl_radius(&p[1].position, a),
               bl_radius(&p[2].position, a), bl_radius(&p[RING].position, a), p[RING].energy,
               p[RING].proper_time, p[RING].active);
    }
    bhrt_particles_destroy(ps);
    particle_system_cleanup(&sys);
    return 0;
}
