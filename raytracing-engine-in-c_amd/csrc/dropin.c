/*
 * dropin.c -- the rest of the reference's entry points: integrate_photon_path, trace_pixel with
 * its sample offsets, and the bh_* context API (src/blackhole_api.c). They keep the reference's
 * argument checks and return codes (src/raytracer.c, src/blackhole_api.c); the tracing itself
 * always runs on the GPU.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "bhrt_host.h"

RayTraceResult integrate_photon_path(const Vector4D* position, const Vector3D* direction,
                                     const BlackHoleParams* bh, const SimulationConfig* cfg,
                                     IntegrationMethod method, Vector3D* path, int max_positions,
                                     int* num_positions, RayTraceHit* hit) {
    if (!position || !direction || bhrt_check_scene(bh, cfg)) return RAY_ERROR;
    int dev = bhrt_current_device();
    devctx_t* c = bhrt_ctx_get(dev);
    if (!c || bhrt_ctx_streams(c)) return RAY_ERROR;
    const int record = path != NULL && num_positions != NULL &&
                       (max_positions > 0 || *num_positions < max_positions);
    const int num_in = (path && max_positions <= 0 && num_positions) ? *num_positions : 0;
    size_t path_bytes = record && max_positions > 0 ? (size_t)max_positions * sizeof(Vector3D) : 0;
    /* layout: [hit SoA: 2 ints + 8 doubles][num][path] */
    size_t need = 128 + 64 + path_bytes;
    if (bhrt_ensure(&c->d_rays, &c->cap_rays, need, 0)) return RAY_ERROR;
    char* d = (char*)c->d_rays;
    bhrt_frame_soa s;
    memset(&s, 0, sizeof s);
    s.result = (int32_t*)d;
    s.steps = (int32_t*)(d + 8);
    s.hit_x = (double*)(d + 16);
    s.hit_y = s.hit_x + 1;
    s.hit_z = s.hit_x + 2;
    s.distance = s.hit_x + 3;
    s.time_dilation = s.hit_x + 4;
    s.sky_x = s.hit_x + 5;
    s.sky_y = s.hit_x + 6;
    s.sky_z = s.hit_x + 7;
    int* d_num = (int*)(d + 128);
    Vector3D* d_path = path_bytes ? (Vector3D*)(d + 192) : NULL;
    bhrt_kparams kp;
    bhrt_fill_scene(&kp, bh, NULL, cfg, method, 0);
    kp.src = BHRT_SRC_RAYS;
    kp.n = 1;
    kp.out = s;
    double o4[4] = {position->t, position->x, position->y, position->z};
    double d3[3] = {direction->x, direction->y, direction->z};
    if (bhrt_launch_path(&kp, o4, d3, d_path, max_positions, d_num, num_in, c->stream) != 0) {
        set_err("path kernel launch failed");
        return RAY_ERROR;
    }
    char h[128 + 64];
    if (hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        set_err("path kernel failed: %s", hipGetErrorString(hipGetLastError()));
        return RAY_ERROR;
    }
    int num = *(int*)(h + 128);
    if (d_path && num > 0) {
        int cnt = num < max_positions ? num : max_positions;
        if (hipMemcpy(path, d_path, (size_t)cnt * sizeof(Vector3D), hipMemcpyDeviceToHost) !=
            hipSuccess) {
            set_err("path readback failed");
            return RAY_ERROR;
        }
    }
    if (path && num_positions && max_positions > 0) *num_positions = num;
    RayTraceResult res = (RayTraceResult)(*(int32_t*)h);
    if (hit) {
        const double* v = (const double*)(h + 16);
        hit->result = res;
        hit->steps = *(int32_t*)(h + 8);
        hit->hit_position.x = v[0];
        hit->hit_position.y = v[1];
        hit->hit_position.z = v[2];
        hit->distance = v[3];
        hit->time_dilation = v[4];
        if (res == RAY_MAX_DISTANCE) {
            hit->sky_direction.x = v[5];
            hit->sky_direction.y = v[6];
            hit->sky_direction.z = v[7];
        }
    }
    return res;
}

/* raytracer.c:868-932 */
void bhrt_jitter(int sample, int spp, JitterMethod jm, double strength, double* ox, double* oy) {
    *ox = 0.5;
    *oy = 0.5;
    switch (jm) {
    case JITTER_REGULAR_GRID: {
        int g = (int)sqrt((double)spp);
        int x = sample % g, y = sample / g;
        *ox = (x + 0.5) / g;
        *oy = (y + 0.5) / g;
    } break;
    case JITTER_RANDOM:
        *ox = (double)rand() / RAND_MAX;
        *oy = (double)rand() / RAND_MAX;
        break;
    case JITTER_HALTON:
    case JITTER_BLUE_NOISE:
        *ox = halton_sequence(sample, 2);
        *oy = halton_sequence(sample, 3);
        break;
    default: break;
    }
    if (strength != 1.0) {
        *ox = 0.5 + (*ox - 0.5) * strength;
        *oy = 0.5 + (*oy - 0.5) * strength;
    }
}

/* raytracer.c:1044-1167: all samples of the pixel are traced in one GPU launch. Disk
 * samples take the frame colour contract's disk colour (the reference reads the never
 * written RayTraceHit.color there). */
RayTraceResult trace_pixel(int px, int py, int W, int H, const Vector3D* cam_pos,
                           const Vector3D* cam_dir, const Vector3D* cam_up, double fov,
                           const BlackHoleParams* bh, const AccretionDiskParams* dk,
                           const SimulationConfig* cfg, const SupersamplingParams* ss,
                           const AdaptiveSamplingParams* as, double color_out[3]) {
    color_out[0] = color_out[1] = color_out[2] = 0.0;
    int samples = ss ? ss->samples_per_pixel : 1;
    if (as && as->enable_adaptive) { /* :1076-1093, edge_factor fixed at 1.0 */
        samples = as->min_samples;
        samples += (int)((as->max_samples - as->min_samples) * 1.0);
        if (samples > as->max_samples) samples = as->max_samples;
    }
    RayTraceResult result = RAY_BACKGROUND;
    if (samples > 0) {
        if (!cam_pos || !cam_dir || !cam_up || bhrt_check_scene(bh, cfg)) return RAY_ERROR;
        Ray* rays = (Ray*)malloc(sizeof(Ray) * (size_t)samples);
        double* rgb = (double*)malloc(sizeof(double) * 3 * (size_t)samples);
        int32_t* res = (int32_t*)malloc(sizeof(int32_t) * (size_t)samples);
        if (!rays || !rgb || !res) {
            free(rays); free(rgb); free(res);
            return RAY_ERROR;
        }
        bhrt_camera cam = {*cam_pos, *cam_dir, *cam_up, fov, 0, 0.0, 0.0};
        bhrt_kparams basis;
        bhrt_fill_scene(&basis, bh, dk, cfg, INTEGRATOR_RK4, 0);
        bhrt_fill_camera(&basis, &cam, W, H);
        for (int s = 0; s < samples; s++) {
            double ox = 0.5, oy = 0.5;
            if (ss && ss->samples_per_pixel > 1)
                bhrt_jitter(s, ss->samples_per_pixel, ss->jitter_method, ss->jitter_strength, &ox, &oy);
            double ndcx = (2.0 * ((px + ox) / W) - 1.0) * basis.cam.plane_w;
            double ndcy = (1.0 - 2.0 * ((py + oy) / H)) * basis.cam.plane_h;
            Vector3D f = {basis.cam.fwd[0], basis.cam.fwd[1], basis.cam.fwd[2]};
            Vector3D r = {basis.cam.right[0], basis.cam.right[1], basis.cam.right[2]};
            Vector3D u = {basis.cam.up[0], basis.cam.up[1], basis.cam.up[2]};
            Vector3D d = vector3D_add(f, vector3D_scale(r, ndcx));
            d = vector3D_add(d, vector3D_scale(u, ndcy));
            rays[s].origin = *cam_pos;
            rays[s].direction = vector3D_normalize(d);
        }
        bhrt_frame_soa soa;
        memset(&soa, 0, sizeof soa);
        soa.result = res;
        soa.rgb_r = rgb;
        soa.rgb_g = rgb + samples;
        soa.rgb_b = rgb + 2 * samples;
        int rc = bhrt_trace_rays(rays, samples, bh, dk, cfg, INTEGRATOR_RK4, 0, &soa);
        if (rc == 0) {
            result = (RayTraceResult)res[0];
            for (int s = 0; s < samples; s++) {
                color_out[0] += soa.rgb_r[s];
                color_out[1] += soa.rgb_g[s];
                color_out[2] += soa.rgb_b[s];
            }
        }
        free(rays); free(rgb); free(res);
        if (rc != 0) return RAY_ERROR;
    }
    color_out[0] /= samples;
    color_out[1] /= samples;
    color_out[2] /= samples;
    return result;
}

/* ======================================================================================= */
/* context API (src/blackhole_api.c)                                                       */
/* ======================================================================================= */
BHContextHandle bh_initialize(void) { /* blackhole_api.c:52-80 */
    BHContextHandle c = (BHContextHandle)calloc(1, sizeof(struct BHContext_t));
    if (!c) return NULL;
    c->blackhole.mass = 1.0;
    c->blackhole.schwarzschild_radius = 2.0;
    c->disk.inner_radius = 6.0;
    c->disk.outer_radius = 20.0;
    c->disk.temperature_scale = 1.0;
    c->disk.density_scale = 1.0;
    c->config.time_step = 0.1;
    c->config.max_ray_distance = 100.0;
    c->config.max_integration_steps = 1000;
    c->config.tolerance = 1.0e-6;
    return c;
}

void bh_shutdown(BHContextHandle c) { free(c); }

double blackhole_get_mass(BHContextHandle c) { return c ? c->blackhole.mass : 0.0; }

void bh_calculate_orbital_velocity(BHContextHandle c, double r, double* v_phi) {
    if (!c || !v_phi || r <= 0) return;
    *v_phi = sqrt(blackhole_get_mass(c) / r);
}

BHErrorCode bh_configure_black_hole(BHContextHandle c, double mass, double spin, double charge) {
    if (!c || mass <= 0.0 || spin < 0.0 || spin > 1.0) return BH_ERROR_INVALID_PARAMETER;
    initialize_black_hole_params(&c->blackhole, mass, spin, charge);
    return BH_SUCCESS;
}

BHErrorCode bh_configure_accretion_disk(BHContextHandle c, double inner, double outer,
                                        double tscale, double density) {
    if (!c || inner <= 0.0 || outer <= inner || tscale <= 0.0 || density <= 0.0)
        return BH_ERROR_INVALID_PARAMETER;
    c->disk.inner_radius = inner;
    c->disk.outer_radius = outer;
    c->disk.temperature_scale = tscale;
    c->disk.density_scale = density;
    c->disk_enabled = 1;
    return BH_SUCCESS;
}

BHErrorCode bh_configure_simulation(BHContextHandle c, double dt, double max_dist, int max_steps,
                                    double tol) {
    if (!c || dt <= 0.0 || max_dist <= 0.0 || max_steps <= 0 || tol <= 0.0)
        return BH_ERROR_INVALID_PARAMETER;
    c->config.time_step = dt;
    c->config.max_ray_distance = max_dist;
    c->config.max_integration_steps = max_steps;
    c->config.tolerance = tol;
    return BH_SUCCESS;
}

BHErrorCode bh_trace_ray(BHContextHandle c, const double origin[3], const double direction[3],
                         RayTraceHit* hit) {
    if (!c || !origin || !direction || !hit) return BH_ERROR_INVALID_PARAMETER;
    Ray ray;
    ray.origin.x = origin[0];
    ray.origin.y = origin[1];
    ray.origin.z = origin[2];
    Vector3D d = {direction[0], direction[1], direction[2]};
    ray.direction = vector3D_normalize(d); /* blackhole_api.c:203-204 */
    RayTraceResult r = trace_ray(&ray, &c->blackhole, c->disk_enabled ? &c->disk : NULL,
                                 &c->config, hit);
    return r == RAY_ERROR ? BH_ERROR_SIMULATION : BH_SUCCESS;
}

BHErrorCode bh_trace_rays_batch(BHContextHandle c, const Ray* rays, RayTraceHit* hits, int count) {
    if (!c || !rays || !hits || count <= 0) return BH_ERROR_INVALID_PARAMETER;
    if (trace_rays_batch(rays, count, &c->blackhole, c->disk_enabled ? &c->disk : NULL,
                         &c->config, hits, 0) != 0)
        return BH_ERROR_SIMULATION;
    for (int i = 0; i < count; i++)
        if (hits[i].result == RAY_ERROR) return BH_ERROR_SIMULATION;
    return BH_SUCCESS;
}

BHErrorCode bh_calculate_time_dilation(BHContextHandle c, const double p1[3], const double p2[3],
                                       double* ratio) {
    if (!c || !p1 || !p2 || !ratio) return BH_ERROR_INVALID_PARAMETER;
    double r1 = sqrt(p1[0] * p1[0] + p1[1] * p1[1] + p1[2] * p1[2]);
    double r2 = sqrt(p2[0] * p2[0] + p2[1] * p2[1] + p2[2] * p2[2]);
    *ratio = calculate_time_dilation(r1, &c->blackhole) / calculate_time_dilation(r2, &c->blackhole);
    return BH_SUCCESS;
}

void bh_get_version(int* major, int* minor, int* patch) {
    if (major) *major = BLACKHOLE_API_VERSION_MAJOR;
    if (minor) *minor = BLACKHOLE_API_VERSION_MINOR;
    if (patch) *patch = BLACKHOLE_API_VERSION_PATCH;
}

/* blackhole_api.c:495-608: packs a float parameter block for a shader */
BHErrorCode bh_generate_shader_data(void* context, const float pos[3], const float dir[3],
                                    const float up[3], int width, int height, float fov,
                                    int enable_doppler, int enable_redshift, int show_disk,
                                    float* out) {
    if (!context || !pos || !dir || !up || !out) return BH_ERROR_INVALID_PARAMETER;
    BHContextHandle c = (BHContextHandle)context;
    struct {
        float mass, spin, schwarzschild_radius, r_isco, r_horizon;
        float disk_inner_radius, disk_outer_radius, disk_temp_scale, disk_density_scale;
        float observer_pos[3], observer_dir[3], up_vector[3];
        float fov, aspect_ratio;
        int enable_doppler, enable_redshift, show_disk;
        int max_steps;
        float step_size, tolerance, max_distance;
        float padding[4];
    } p;
    p.mass = (float)c->blackhole.mass;
    p.spin = (float)c->blackhole.spin;
    p.schwarzschild_radius = (float)c->blackhole.schwarzschild_radius;
    p.r_isco = (float)c->blackhole.isco_radius;
    p.r_horizon = (float)c->blackhole.r_plus;
    int disk_on = show_disk && c->disk_enabled;
    p.disk_inner_radius = disk_on ? (float)c->disk.inner_radius : 1000.0f;
    p.disk_outer_radius = disk_on ? (float)c->disk.outer_radius : 100.0f;
    p.disk_temp_scale = disk_on ? (float)c->disk.temperature_scale : 0.0f;
    p.disk_density_scale = disk_on ? (float)c->disk.density_scale : 0.0f;
    memcpy(p.observer_pos, pos, sizeof p.observer_pos);
    memcpy(p.observer_dir, dir, sizeof p.observer_dir);
    memcpy(p.up_vector, up, sizeof p.up_vector);
    p.fov = fov * (float)BH_PI / 180.0f;
    p.aspect_ratio = (float)width / (float)height;
    p.enable_doppler = enable_doppler;
    p.enable_redshift = enable_redshift;
    p.show_disk = disk_on;
    p.max_steps = c->config.max_integration_steps;
    p.step_size = (float)c->config.time_step;
    p.tolerance = (float)c->config.tolerance;
    p.max_distance = (float)c->config.max_ray_distance;
    memset(p.padding, 0, sizeof p.padding);
    memcpy(out, &p, sizeof p);
    return BH_SUCCESS;
}
