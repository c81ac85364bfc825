/*
 * oracle/ref_probe/path_probe.cpp -- TEST INFRASTRUCTURE.
 *
 * Runs the REFERENCE's own loader, BVH builder, traversal, light sampling,
 * integrator and pixel kernel on the CPU: its headers are compiled from where
 * they lie ($(REF)/include, and the part of Render.cuh before its Render class,
 * which oracle/Makefile cuts into oracle/_ref/), against the stand-in CUDA and
 * cuRAND headers of standin/ and the deterministic libm of det_libm.cpp.
 * Nothing of the reference is copied here; this file only calls it.
 *
 *   path_probe MODE job.bin out.bin          MODE = scene | intersect | paths | frame | samplers
 *
 * samplers (no scene): job.bin = u32 n_w, f32 a[n_w][3], f32 N[n_w][3], u32 n_h, f32 N[n_h][3], u32 tape[n_h][2], u32 n_l,
 *   f32 (out[3], delta_theta, delta_phi)[n_l], u32 tape[n_l][2];  out.bin = f32 to_world[n_w][3], f32 get_cuda_random_sphere_vector[n_h][3],
 *   f32 get_cuda_random_specular_sphere_vector[n_l][3]   (Global.h:35-94)
 * every other mode:
 * job.bin (little-endian):  u32 n_obj, n_obj x { u32 len, OBJ path, u32 len, MTL dir }, u32 bvh_thresh_n, then
 *   scene      --
 *   intersect  u32 n, f32 origin[n][3], f32 dir[n][3], f32 limit[n]
 *   paths      u32 n, f32 P_RR, i32 light_sample_n, f32 ray[n][6] (origin, direction as handed to Ray), u64 off[n+1], u32 tape[off[n]]
 *   frame      u32 width, height, spp, f32 P_RR, i32 light_sample_n, f32 eye[3], f32 inv_view[9] (column-major), f32 fov_y,
 *              u32 n, u32 pixel[n] (j * width + i), u64 off[n+1], u32 tape[off[n]]   (one tape per listed pixel, jitter included)
 * out.bin:
 *   scene      u32 n_nodes, i32 root, u32 n_tris, u32 n_lights, node[n_nodes] (lc rc n it AA BB), tri[n_tris] in BVH order,
 *              n_lights x { u32 n, tri[n] in shape order };  tri = v1 v2 v3 e1 e2 normal kd ke ns has_emit mode area area_of_obj
 *   intersect  n x { i32 happend, f32 t, f32 pos[3], f32 normal[3], i32 triangle, i32 blocked(limit), i32 triangles that match }
 *   paths      n x { f32 L[3], u32 words consumed }
 *   frame      u8 rgb[n][3], u64 words consumed[n]
 * Exit status 3: a tape ran out (standin/curand_kernel.h); 2: bad job.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Eigen/Dense"
#include "cuda_runtime.h"
#include "curand_kernel.h"

uint3 blockIdx = {0, 0, 0}, threadIdx = {0, 0, 0};
dim3 blockDim(1, 1, 1), gridDim(1, 1, 1);
ref_tape g_ref_tape = {nullptr, 0, 0};

/* the reference's classes keep what the probe has to dump in private members */
#define private public
#include "Loader.h"
#include "Object.h"
#include "Scene.h"
#include "BVH.h"
#include "Render_head.cuh"
#undef private

namespace {

struct Job {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    void need(size_t n) const
    {
        if (pos + n > buf.size()) { std::fprintf(stderr, "path_probe: job file is too short\n"); std::exit(2); }
    }
    template <typename T> T get()
    {
        T v;
        need(sizeof(T));
        std::memcpy(&v, buf.data() + pos, sizeof(T));
        pos += sizeof(T);
        return v;
    }
    template <typename T> std::vector<T> array(size_t n)
    {
        std::vector<T> v(n);
        need(n * sizeof(T));
        if (n) std::memcpy(v.data(), buf.data() + pos, n * sizeof(T));
        pos += n * sizeof(T);
        return v;
    }
    std::string str()
    {
        uint32_t n = get<uint32_t>();
        need(n);
        std::string s((const char*)buf.data() + pos, n);
        pos += n;
        return s;
    }
};

struct Out {
    FILE* f;
    template <typename T> void put(const T& v) { std::fwrite(&v, sizeof(T), 1, f); }
    void vec(const Eigen::Vector3f& v) { float a[3] = {v.x(), v.y(), v.z()}; std::fwrite(a, 4, 3, f); }
};

void put_tri(Out& o, DeviceTriangle& t)
{
    o.vec(t.v1); o.vec(t.v2); o.vec(t.v3); o.vec(t.e1); o.vec(t.e2); o.vec(t.normal);
    o.vec(t.device_material.kd); o.vec(t.device_material.ke);
    o.put<float>(t.device_material.ns);
    o.put<int32_t>(t.device_material.has_emit ? 1 : 0);
    o.put<int32_t>((int32_t)t.device_material.mode);
    o.put<float>(t.area);
    o.put<float>(t.area_of_obj);
}

uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

} // namespace

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: path_probe scene|intersect|paths|frame job.bin out.bin\n"); return 2; }
    const std::string mode = argv[1];
    Job job;
    {
        std::ifstream in(argv[2], std::ios::binary);
        if (!in) { std::fprintf(stderr, "path_probe: cannot read %s\n", argv[2]); return 2; }
        job.buf.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    }
    if (mode == "samplers") {
        /* Global.h:35-94 at chosen inputs; no scene.  The two tape words of a record are what its two curand_uniform calls read. */
        Out out{std::fopen(argv[3], "wb")};
        if (!out.f) { std::fprintf(stderr, "path_probe: cannot write %s\n", argv[3]); return 2; }
        const uint32_t n_w = job.get<uint32_t>();
        const std::vector<float> wa = job.array<float>(3 * (size_t)n_w), wn = job.array<float>(3 * (size_t)n_w);
        const uint32_t n_h = job.get<uint32_t>();
        const std::vector<float> hn = job.array<float>(3 * (size_t)n_h);
        const std::vector<uint32_t> hw = job.array<uint32_t>(2 * (size_t)n_h);
        const uint32_t n_l = job.get<uint32_t>();
        const std::vector<float> lr = job.array<float>(5 * (size_t)n_l);
        const std::vector<uint32_t> lw = job.array<uint32_t>(2 * (size_t)n_l);
        curandState st;
        for (uint32_t i = 0; i < n_w; i++)
            out.vec(to_world(Eigen::Vector3f(wa[3 * i], wa[3 * i + 1], wa[3 * i + 2]), Eigen::Vector3f(wn[3 * i], wn[3 * i + 1], wn[3 * i + 2])));
        for (uint32_t i = 0; i < n_h; i++) {
            ref_tape_select(hw.data() + 2 * (size_t)i, 2);
            curand_init(0, 0, 0, &st);
            out.vec(get_cuda_random_sphere_vector(Eigen::Vector3f(hn[3 * i], hn[3 * i + 1], hn[3 * i + 2]), &st));
        }
        for (uint32_t i = 0; i < n_l; i++) {
            ref_tape_select(lw.data() + 2 * (size_t)i, 2);
            curand_init(0, 0, 0, &st);
            const float* r = &lr[5 * (size_t)i];
            out.vec(get_cuda_random_specular_sphere_vector(Eigen::Vector3f(r[0], r[1], r[2]), r[3], r[4], &st));
        }
        if (std::fclose(out.f) != 0) return 2;
        return 0;
    }
    /* the scene, through the reference's Loader, Object and Scene, in the order its render_view() adds objects */
    Scene scene(1, 1);
    const uint32_t n_obj = job.get<uint32_t>();
    for (uint32_t k = 0; k < n_obj; k++) {
        const std::string obj = job.str(), mtl = job.str();
        Loader loader;
        std::vector<Triangle> tris, light_tris;
        loader.read_OBJ(obj.c_str(), mtl.c_str());
        for (uint64_t i = 0; i < loader.size(); i++) {
            loader.load_object(i, tris, light_tris);
            if (tris.size() > 0) { Object o(tris); scene.add_normal_obj(o); }
            if (light_tris.size() > 0) { Object o(light_tris); scene.add_light_obj(o); }
        }
    }
    scene.set_BVH(job.get<uint32_t>());
    DeviceBVH dbvh(scene.get_bvh());
    DeviceLights dlights(scene.get_light_objs());
    auto* bvh_stack = new DeviceStack<int, BVH_STACK_SIZE>();

    Out out{std::fopen(argv[3], "wb")};
    if (!out.f) { std::fprintf(stderr, "path_probe: cannot write %s\n", argv[3]); return 2; }

    if (mode == "scene") {
        const uint32_t n_nodes = (uint32_t)scene.get_bvh().get_nodes_size(), n_tris = (uint32_t)scene.get_bvh().get_triangles_size();
        out.put<uint32_t>(n_nodes);
        out.put<int32_t>((int32_t)*dbvh.root_index);
        out.put<uint32_t>(n_tris);
        out.put<uint32_t>((uint32_t)*dlights.ln);
        for (uint32_t i = 0; i < n_nodes; i++) {
            DeviceBVHNode& n = dbvh.nodes[i];
            out.put<int32_t>(n.lc); out.put<int32_t>(n.rc); out.put<uint32_t>(n.n); out.put<int32_t>(n.it);
            out.vec(n.AA); out.vec(n.BB);
        }
        for (uint32_t i = 0; i < n_tris; i++) put_tri(out, dbvh.triangles[i]);
        for (size_t l = 0; l < *dlights.ln; l++) {
            DeviceLight& dl = dlights.dls[l];
            out.put<uint32_t>((uint32_t)*dl.tn);
            for (size_t i = 0; i < *dl.tn; i++) put_tri(out, dl.dts[i]);
        }
    } else if (mode == "intersect") {
        const uint32_t n = job.get<uint32_t>();
        const std::vector<float> o = job.array<float>(3 * (size_t)n), d = job.array<float>(3 * (size_t)n), lim = job.array<float>(n);
        const uint32_t n_tris = (uint32_t)scene.get_bvh().get_triangles_size();
        for (uint32_t i = 0; i < n; i++) {
            Ray ray(Eigen::Vector3f(o[3 * i], o[3 * i + 1], o[3 * i + 2]), Eigen::Vector3f(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
            HitPayload h = dbvh.intersect(ray.get_origin(), ray.get_dir(), ray.get_inv_dir(), bvh_stack);
            const bool blk = blocked(ray, lim[i], &dbvh, bvh_stack);
            /* which triangle: the ones whose own get_intersection gives this very hit */
            int32_t tri = -1, matches = 0;
            if (h.happend) {
                for (uint32_t k = 0; k < n_tris; k++) {
                    const Eigen::Vector3f& nk = dbvh.triangles[k].normal; /* (a triangle with another normal cannot match: skip its test) */
                    if (fbits(nk.x()) != fbits(h.normal.x()) || fbits(nk.y()) != fbits(h.normal.y()) || fbits(nk.z()) != fbits(h.normal.z())) continue;
                    HitPayload g = dbvh.triangles[k].get_intersection(ray.get_origin(), ray.get_dir());
                    if (g.happend && fbits(g.t) == fbits(h.t) && fbits(g.pos.x()) == fbits(h.pos.x()) && fbits(g.pos.y()) == fbits(h.pos.y()) &&
                        fbits(g.pos.z()) == fbits(h.pos.z()) && fbits(g.normal.x()) == fbits(h.normal.x()) &&
                        fbits(g.normal.y()) == fbits(h.normal.y()) && fbits(g.normal.z()) == fbits(h.normal.z())) {
                        if (tri < 0) tri = (int32_t)k;
                        matches++;
                    }
                }
            }
            out.put<int32_t>(h.happend ? 1 : 0);
            out.put<float>(h.t);
            out.vec(h.pos); out.vec(h.normal);
            out.put<int32_t>(tri);
            out.put<int32_t>(blk ? 1 : 0);
            out.put<int32_t>(matches);
        }
    } else if (mode == "paths") {
        const uint32_t n = job.get<uint32_t>();
        const float p_rr = job.get<float>();
        const int32_t lsn = job.get<int32_t>();
        const std::vector<float> rays = job.array<float>(6 * (size_t)n);
        const std::vector<uint64_t> off = job.array<uint64_t>((size_t)n + 1);
        const std::vector<uint32_t> tape = job.array<uint32_t>(off[n]);
        auto* bounce = new DeviceStack<HitPayload, BOUNCE_STACK_SIZE>();
        for (uint32_t i = 0; i < n; i++) {
            ref_tape_select(tape.data() + off[i], off[i + 1] - off[i]);
            curandState st;
            curand_init(0, 0, 0, &st);
            const float* r = &rays[6 * (size_t)i];
            Ray ray(Eigen::Vector3f(r[0], r[1], r[2]), Eigen::Vector3f(r[3], r[4], r[5]));
            Eigen::Vector3f L = cast_ray_v2(ray, 0, lsn, p_rr, &st, &dbvh, &dlights, bounce, bvh_stack);
            out.vec(L);
            out.put<uint32_t>((uint32_t)g_ref_tape.pos);
        }
    } else if (mode == "frame") {
        const uint32_t w = job.get<uint32_t>(), h = job.get<uint32_t>(), spp = job.get<uint32_t>();
        const float p_rr = job.get<float>();
        const int32_t lsn = job.get<int32_t>();
        const std::vector<float> eye = job.array<float>(3), iv = job.array<float>(9);
        const float fov_y = job.get<float>();
        const size_t px = (size_t)w * h;
        const uint32_t n = job.get<uint32_t>();
        const std::vector<uint32_t> pixel = job.array<uint32_t>(n);
        const std::vector<uint64_t> off = job.array<uint64_t>((size_t)n + 1);
        const std::vector<uint32_t> tape = job.array<uint32_t>(off[n]);
        Eigen::Matrix3f inv_view;
        for (int c = 0; c < 3; c++)
            for (int r = 0; r < 3; r++) inv_view(r, c) = iv[3 * c + r];
        std::vector<uchar3> frame(px);
        std::vector<uint64_t> used(n);
        /* the kernel indexes its stacks and its frame buffer by pixel: whole-frame arrays */
        auto* bounce = new DeviceStack<HitPayload, BOUNCE_STACK_SIZE>[px];
        auto* stacks = new DeviceStack<int, BVH_STACK_SIZE>[px];
        blockDim = dim3(1, 1, 1);
        for (uint32_t q = 0; q < n; q++) {
            if (pixel[q] >= px) { std::fprintf(stderr, "path_probe: pixel outside the frame\n"); return 2; }
            ref_tape_select(tape.data() + off[q], off[q + 1] - off[q]);
            blockIdx = {pixel[q] % w, pixel[q] / w, 0};
            threadIdx = {0, 0, 0};
            view_render_kernel(w, h, Eigen::Vector3f(eye[0], eye[1], eye[2]), inv_view, fov_y, spp, p_rr, lsn, &dbvh, frame.data(), &dlights, bounce,
                               stacks);
            used[q] = g_ref_tape.pos;
        }
        for (uint32_t q = 0; q < n; q++) { const uchar3 c = frame[pixel[q]]; out.put<uint8_t>(c.x); out.put<uint8_t>(c.y); out.put<uint8_t>(c.z); }
        for (uint32_t q = 0; q < n; q++) out.put<uint64_t>(used[q]);
    } else {
        std::fprintf(stderr, "path_probe: unknown mode %s\n", mode.c_str());
        return 2;
    }
    if (std::fclose(out.f) != 0) return 2;
    return 0;
}
