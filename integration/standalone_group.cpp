/*
 * standalone_group.cpp — the headless render loop of standalone_cornell.cpp
 * (Standalone/StandaloneRenderManager.cpp:55-140) driving N ranks through the render-group API
 * of include/orx.h: no Python, no collective of the caller's.  Plain C++, liborx.so only.
 *
 *   standalone_group --ranks N [--devices a,b,..] --partition rows|batch --comm auto|local|rccl
 *                    [--photons rows|slabs] [--serial] --method ppm|pt|vcm --width W --height H
 *                    --photon-launch P --iterations I --seed S --out output.f32
 *                    [--save-state FILE] [--load-state FILE]
 *                    [--until-error E [--error-floor F]] [--display FILE]
 *
 * --devices defaults to device 0 for every rank (the one-device LOCAL communicator).  rows: I
 * iterations of one frame over the ranks; batch: I iterations dealt round-robin to the ranks.
 * --photons slabs (with --partition rows): PPM frames exchange photons by spatial slab, so each
 * rank gathers only the hit points of its slab (orx_group_config.photon_partition); default rows.
 * Writes the W*H*3 float running sum to --out.  --save-state writes the group's state blob after the last
 * iteration; --load-state restores one before the first, and the I iterations go on from its header.
 * --until-error E (rows partition) stops at the first iteration >= 2 whose mean error
 * (orx_group_get_convergence, denominator floor F, default 1e-3) is <= E, or at I, and prints
 * "iterations n mean_error x"; --display writes the frame as BGRA8 at gamma 2.2 (W*H*4 bytes).
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "orx.h"

/* Cornell.cpp:20-207 as flat arrays: five Lambert walls and an area light under the ceiling */
struct Cornell {
    std::vector<float> quads;
    std::vector<uint32_t> qmat;
    std::vector<orx_material> mats;
    orx_light light;
    float mn[3], mx[3];

    Cornell() {
        const float lp[3] = {343.0f, 548.7999f, 227.0f}, lv1[3] = {0.0f, 0.0f, 105.0f}, lv2[3] = {-130.0f, 0.0f, 0.0f};
        const float pw[3] = {0.5e6f, 0.4e6f, 0.2e6f};
        light = orx_light{};
        light.type = ORX_LIGHT_AREA;
        for (int k = 0; k < 3; k++) {
            light.power[k] = pw[k];
            light.position[k] = lp[k];
            light.v1[k] = lv1[k];
            light.v2[k] = lv2[k];
        }
        /* Light.cpp:14-28: inverse area 1/|v1 x v2| in float */
        const float cx = lv1[1] * lv2[2] - lv1[2] * lv2[1], cy = lv1[2] * lv2[0] - lv1[0] * lv2[2],
                    cz = lv1[0] * lv2[1] - lv1[1] * lv2[0];
        const float inv_area = 1.0f / std::sqrt((cx * cx + cy * cy) + cz * cz);
        const uint32_t white = material(0.8f, 0.8f, 0.8f), green = material(0.05f, 0.8f, 0.05f),
                       red = material(1.0f, 0.05f, 0.05f);
        quad(0, 0, 0, 0, 0, 559.2f, 556.0f, 0, 0, white);       /* floor */
        quad(0, 548.80f, 0, 556.0f, 0, 0, 0, 0, 559.2f, white); /* ceiling */
        quad(0, 0, 559.2f, 0, 548.8f, 0, 556.0f, 0, 0, white);  /* back wall */
        quad(0, 0, 0, 0, 548.8f, 0, 0, 0, 559.2f, green);       /* right wall */
        quad(556.0f, 0, 0, 0, 0, 559.2f, 0, 548.8f, 0, red);    /* left wall */
        orx_material em = {};
        em.type = ORX_MAT_DIFFUSE_EMITTER;
        for (int k = 0; k < 3; k++) {
            em.Kd[k] = 1.0f;
            em.power[k] = pw[k];
        }
        em.inverse_area = inv_area;
        em.texture = -1;
        mats.push_back(em);
        quad(lp[0], lp[1], lp[2], lv1[0], lv1[1], lv1[2], lv2[0], lv2[1], lv2[2], (uint32_t)mats.size() - 1);
        const float hi[3] = {556.0f, 548.85f, 559.2f}; /* Cornell.cpp:28-31 */
        for (int k = 0; k < 3; k++) {
            mn[k] = -5.0f;
            mx[k] = hi[k] + 5.0f;
        }
    }
    orx_scene flat() const {
        orx_scene s = {};
        s.n_quads = (uint32_t)qmat.size();
        s.quads = quads.data();
        s.quad_material = qmat.data();
        s.n_materials = (uint32_t)mats.size();
        s.materials = mats.data();
        s.n_lights = 1;
        s.lights = &light;
        for (int k = 0; k < 3; k++) {
            s.aabb_min[k] = mn[k];
            s.aabb_max[k] = mx[k];
        }
        return s;
    }
    /* IScene.cpp:51-59: A * 3.94e-6, A = 6 * cbrt(V)^2 over the scene AABB */
    float initial_radius() const {
        const float ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
        const float volume = (ex * ey) * ez;
        const float cube = (float)std::pow((double)volume, 1.0 / 3.0);
        const float A = (6.0f * cube) * cube;
        return (float)((double)A * 3.94e-6);
    }
    /* Cornell.cpp:199-207 with Camera::setAspectRatio (Camera.cpp:294-318, vertical fov kept) */
    orx_camera camera(float ratio) const {
        orx_camera c = {};
        const float eye[3] = {278.0f, 273.0f, -850.0f}, at[3] = {278.0f, 273.0f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
        for (int k = 0; k < 3; k++) {
            c.eye[k] = eye[k];
            c.lookat[k] = at[k];
            c.up[k] = up[k];
        }
        c.vfov = 35.0f;
        const float d2r = (float)M_PI / 180.0f, r2d = 180.0f / (float)M_PI;
        const float t = (float)std::tan((double)((0.5f * c.vfov) * d2r));
        c.hfov = (2.0f * (float)std::atan((double)(ratio * t))) * r2d;
        c.aperture = 0.0f;
        return c;
    }

private:
    uint32_t material(float r, float g, float b) {
        orx_material m = {};
        m.type = ORX_MAT_DIFFUSE;
        m.Kd[0] = r;
        m.Kd[1] = g;
        m.Kd[2] = b;
        m.ior = 1.0f;
        m.exponent = 1.0f;
        m.texture = -1;
        mats.push_back(m);
        return (uint32_t)mats.size() - 1;
    }
    void quad(float ax, float ay, float az, float ux, float uy, float uz, float vx, float vy, float vz, uint32_t mat) {
        const float q[9] = {ax, ay, az, ux, uy, uz, vx, vy, vz};
        quads.insert(quads.end(), q, q + 9);
        qmat.push_back(mat);
    }
};

static std::vector<unsigned char> read_file(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    std::vector<unsigned char> data;
    unsigned char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    return data;
}

static void check(orx_group* g, orx_status s, const char* what) {
    if (s == ORX_OK) return;
    const char* m = orx_group_last_error(g);
    throw std::runtime_error(std::string(what) + ": " + (m && *m ? m : "failed") + " (status " + std::to_string((int)s) + ")");
}

int main(int argc, char** argv) {
    const char *method = "ppm", *out = nullptr, *partition = "rows", *comm = "auto", *devices = nullptr, *photons = "rows";
    const char *save_state = nullptr, *load_state = nullptr, *display = nullptr;
    bool until = false;
    float until_error = 0.f, error_floor = 1e-3f;
    unsigned W = 32, H = 32, P = 64, iters = 2, seed = 1645301512u, ranks = 1;
    bool serial = false;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--serial")) {
            serial = true;
            continue;
        }
        if (i + 1 >= argc) break;
        if (!std::strcmp(argv[i], "--method")) method = argv[++i];
        else if (!std::strcmp(argv[i], "--ranks")) ranks = (unsigned)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--devices")) devices = argv[++i];
        else if (!std::strcmp(argv[i], "--partition")) partition = argv[++i];
        else if (!std::strcmp(argv[i], "--comm")) comm = argv[++i];
        else if (!std::strcmp(argv[i], "--photons")) photons = argv[++i];
        else if (!std::strcmp(argv[i], "--width")) W = (unsigned)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--height")) H = (unsigned)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--photon-launch")) P = (unsigned)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--iterations")) iters = (unsigned)std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--seed")) seed = (unsigned)std::strtoul(argv[++i], nullptr, 10);
        else if (!std::strcmp(argv[i], "--out")) out = argv[++i];
        else if (!std::strcmp(argv[i], "--save-state")) save_state = argv[++i];
        else if (!std::strcmp(argv[i], "--load-state")) load_state = argv[++i];
        else if (!std::strcmp(argv[i], "--display")) display = argv[++i];
        else if (!std::strcmp(argv[i], "--error-floor")) error_floor = (float)std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--until-error")) {
            until = true;
            until_error = (float)std::atof(argv[++i]);
        }
    }
    orx_group* g = nullptr;
    int rc = 0;
    try {
        const int32_t m = !std::strcmp(method, "pt")    ? ORX_METHOD_PATH_TRACING
                          : !std::strcmp(method, "vcm") ? ORX_METHOD_VCM_BIDIRECTIONAL_PATH_TRACING
                                                        : ORX_METHOD_PROGRESSIVE_PHOTON_MAPPING;
        std::vector<int> devs;
        if (devices)
            for (const char* p = devices; *p;) {
                devs.push_back(std::atoi(p));
                p = std::strchr(p, ',');
                if (!p) break;
                p++;
            }
        else
            devs.assign(ranks, 0);
        if (devs.size() != ranks) throw std::runtime_error("--devices needs one entry per rank");
        orx_config cfg;
        orx_default_config(&cfg);
        cfg.photon_launch_width = cfg.photon_launch_height = P;
        cfg.seed = seed;
        orx_group_config gc;
        orx_default_group_config(&gc);
        if (!std::strcmp(partition, "rows")) gc.partition = ORX_GROUP_ROWS;
        else if (!std::strcmp(partition, "batch")) gc.partition = ORX_GROUP_BATCH;
        else throw std::runtime_error("--partition rows|batch");
        if (!std::strcmp(comm, "auto")) gc.comm = ORX_COMM_AUTO;
        else if (!std::strcmp(comm, "local")) gc.comm = ORX_COMM_LOCAL;
        else if (!std::strcmp(comm, "rccl")) gc.comm = ORX_COMM_RCCL;
        else throw std::runtime_error("--comm auto|local|rccl");
        if (!std::strcmp(photons, "rows")) gc.photon_partition = ORX_PHOTONS_ROWS;
        else if (!std::strcmp(photons, "slabs")) gc.photon_partition = ORX_PHOTONS_SLABS;
        else throw std::runtime_error("--photons rows|slabs");
        gc.pipeline = serial ? 0u : 1u;
        check(nullptr, orx_create_group(ranks, devs.data(), &cfg, &gc, &g), "orx_create_group");
        std::printf("communicator %s world %u partition %s photon-partition %s\n", orx_group_comm_name(g), orx_group_world(g),
                    partition, photons);
        Cornell scene;
        const orx_scene flat = scene.flat();
        check(g, orx_group_init_scene(g, &flat), "orx_group_init_scene");
        const double alpha = 2.0 / 3.0;
        orx_request req = {};
        req.camera = scene.camera((float)W / (float)H);
        req.method = m;
        req.width = W;
        req.height = H;
        req.ppm_alpha = alpha;
        double radius = scene.initial_radius();
        unsigned long long first = 0;
        if (load_state) { /* the iteration after the header's, with the radius that follows the header's */
            const std::vector<unsigned char> blob = read_file(load_state);
            orx_state_info info;
            if (orx_state_info_read(blob.data(), blob.size(), &info) != ORX_OK) throw std::runtime_error("not a state blob");
            check(g, orx_group_restore_state(g, blob.data(), blob.size()), "orx_group_restore_state");
            first = info.iteration_number + 1;
            radius = std::sqrt((double)info.ppm_radius * (double)info.ppm_radius *
                               ((double)info.iteration_number + alpha) / ((double)info.iteration_number + 1.0));
        }
        if (until) check(g, orx_group_set_convergence(g, 1), "orx_group_set_convergence");
        unsigned done = 0;
        float mean_error = 0.f;
        for (unsigned long long it = first; it < first + iters; it++) {
            check(g, orx_group_render_next_iteration(g, it, it, (float)radius, 1, &req), "orx_group_render_next_iteration");
            /* StandaloneRenderManager.cpp:105-107 */
            const double r2 = radius * radius * ((double)it + alpha) / ((double)it + 1.0);
            radius = std::sqrt(r2);
            done++;
            if (until && done >= 2) {
                orx_convergence c;
                check(g, orx_group_get_convergence(g, error_floor, until_error, &c, nullptr, 0), "orx_group_get_convergence");
                mean_error = c.mean_error;
                if (mean_error <= until_error) break;
            }
        }
        if (until) std::printf("iterations %u mean_error %.9g\n", done, mean_error);
        std::vector<float> img((size_t)W * H * 3);
        check(g, orx_group_get_output(g, img.data(), img.size() * sizeof(float)), "orx_group_get_output");
        if (out) {
            FILE* f = std::fopen(out, "wb");
            if (!f || std::fwrite(img.data(), sizeof(float), img.size(), f) != img.size())
                throw std::runtime_error("cannot write output");
            std::fclose(f);
        }
        if (display) { /* the running sum over the iteration count (RenderWidget.cpp:197) */
            std::vector<unsigned char> px((size_t)W * H * 4);
            check(g, orx_group_get_display(g, 1.0f / (float)(first + done), 1.0f / 2.2f, ORX_DISPLAY_BGRA8, px.data(), px.size()),
                  "orx_group_get_display");
            FILE* f = std::fopen(display, "wb");
            if (!f || std::fwrite(px.data(), 1, px.size(), f) != px.size()) throw std::runtime_error("cannot write display");
            std::fclose(f);
        }
        if (save_state) {
            std::vector<unsigned char> blob(orx_group_state_bytes(g) + 1);
            check(g, orx_group_save_state(g, blob.data(), blob.size() - 1), "orx_group_save_state");
            FILE* f = std::fopen(save_state, "wb");
            if (!f || std::fwrite(blob.data(), 1, blob.size() - 1, f) != blob.size() - 1)
                throw std::runtime_error("cannot write state");
            std::fclose(f);
        }
        double sum = 0;
        for (float v : img) sum += v;
        std::printf("ok %s %ux%u photons %u iterations %u pipelined %d mean %.9g\n", method, W, H,
                    orx_emitted_photons_per_iteration(orx_group_renderer(g, 0)), done, orx_group_pipelined(g),
                    sum / (double)img.size());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        rc = 1;
    }
    orx_group_destroy(g);
    return rc;
}
