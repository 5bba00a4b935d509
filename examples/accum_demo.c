/*
 * accum_demo.c -- a disk image that sharpens frame by frame, from a plain C caller of libbhrt.so:
 * one jittered sample per pixel per frame, blended on the GPU by a temporal accumulator
 * (bhrt_accum_create / bhrt_accum_frame), with a camera move in the middle.
 *
 *   gcc -std=c99 -Iinclude examples/accum_demo.c -Lraytracing-engine-in-c_amd -lbhrt \
 *       -Wl,-rpath,$PWD/raytracing-engine-in-c_amd -lm -o accum_demo && ./accum_demo > disk.ppm
 *
 * The scene: a Schwarzschild hole with a disk from 6 M to 20 M, RK4, 320 x 180, the 8 Halton
 * offsets of trace_pixel's jitter. 12 frames from one camera, then the camera moves -- the viewer
 * calls bhrt_accum_reset -- and 12 more. Each frame's state goes to stderr (the blend weight,
 * the offset, how many pixels the edge detector marks); the last display image to stdout as a
 * binary PPM.
 */
#include <stdio.h>
#include <stdlib.h>

#include "blackhole_api.h"

enum { W = 320, H = 180, FRAMES = 24, MOVE_AT = 12 };

int main(void) {
    BlackHoleParams bh;
    initialize_black_hole_params(&bh, 1.0, 0.0, 0.0);
    AccretionDiskParams disk = {0};
    disk.inner_radius = 6.0;
    disk.outer_radius = 20.0;
    disk.temperature_scale = 1.0;
    disk.density_scale = 1.0;
    SimulationConfig cfg = {0};
    cfg.time_step = 0.1;
    cfg.max_ray_distance = 100.0;
    cfg.max_integration_steps = 1000;
    cfg.tolerance = 1e-6;
    bhrt_camera cam = {0};
    cam.position.y = -29.544;
    cam.position.z = 5.209;
    cam.direction.y = 29.544;
    cam.direction.z = -5.209;
    cam.up.z = 1.0;
    cam.fov_deg = 60.0;
    SupersamplingParams ss = {0};
    ss.samples_per_pixel = 8;
    ss.jitter_method = JITTER_HALTON;
    ss.jitter_strength = 1.0;

    static uint8_t rgba8[W * H * 4];
    static float edge[W * H];
    bhrt_accum* acc = NULL;
    if (bhrt_accum_create(W, H, NULL, NULL, &acc) != 0) { /* NULL: initTemporalBuffer's defaults */
        fprintf(stderr, "bhrt_accum_create: %s\n", bhrt_last_error());
        return 1;
    }
    bhrt_accum_out out = {0};
    out.rgba8 = rgba8;
    out.edge_factor = edge;
    for (int k = 0; k < FRAMES; k++) {
        if (k == MOVE_AT) { /* a camera move: the next frame starts a new image */
            cam.position.z = 8.0;
            cam.direction.z = -8.0;
            bhrt_accum_reset(acc);
        }
        bhrt_accum_state st;
        bhrt_accum_info(acc, &ss, &st);
        if (bhrt_accum_frame(acc, &bh, &disk, &cfg, &cam, INTEGRATOR_RK4, 0, &ss, &out) != 0) {
            fprintf(stderr, "bhrt_accum_frame: %s\n", bhrt_last_error());
            bhrt_accum_destroy(acc);
            return 1;
        }
        int edges = 0;
        for (int i = 0; i < W * H; i++) edges += edge[i] == 1.0f;
        fprintf(stderr, "frame %2d: alpha %.2f at offset (%.4f, %.4f), %d edge pixels\n", k,
                (double)st.next_alpha, st.next_offset_x, st.next_offset_y, edges);
    }
    bhrt_accum_destroy(acc);
    printf("P6\n%d %d\n255\n", W, H);
    for (int i = 0; i < W * H; i++) fwrite(rgba8 + 4 * (size_t)i, 1, 3, stdout);
    return 0;
}
