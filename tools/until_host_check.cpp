// tools/until_host_check.cpp -- crt::Render::run_view_until and crt::Render::frame_error (cudaraytracing_amd/csrc/crt_host.hpp) against
// the library calls they are made of.  Needs a GPU.  The scene of the config at 64 x 48, spp 32, seed 0, with the until settings of the
// command line: the method's frame, mean, variance and figures are compared bit for bit with crt_render_until made directly on a second
// scene handle, the summary with crt_frame_error; then both handles continue their frame with threshold 0 to spp, where the frame must
// be crt_render's of a third handle.  Exits 1 at the first mismatch with one line that names the comparison.  Writes the samples done
// (uint32), the RGB8 frame and the mean of the first call to <out>, for the caller to compare with its own.
//
//   cudaraytracing_amd/build.py builds it beside crt_cli, as lib/until_host_check
//   until_host_check scenes/cornell-box/config.json <base dir of the OBJ paths> THRESHOLD MAX_ABOVE MIN STEP <out>
#include "../cudaraytracing_amd/csrc/crt_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

const uint32_t W = 64, H = 48, S = 32;
const size_t N = (size_t)W * H;

[[noreturn]] void fail(const std::string& what)
{
    std::fprintf(stderr, "until_host_check: %s\n", what.c_str());
    std::exit(1);
}
void ok(int rc, const char* call) { if (rc != CRT_OK) fail(std::string(call) + " failed: " + crt_last_error()); }
template <class T> void same(const std::string& what, const T* a, const T* b, size_t n)
{
    if (std::memcmp(a, b, n * sizeof(T)) != 0) fail(what + " differs");
}
void same_info(const std::string& what, const crt_until_info& a, const crt_until_info& b)
{
    if (a.passes != b.passes || a.checks != b.checks || a.samples_done != b.samples_done || a.paths != b.paths || std::memcmp(a.above, b.above, sizeof(a.above)) != 0 ||
        std::memcmp(&a.last, &b.last, sizeof(a.last)) != 0)
        fail(what + ": last_until_info differs");
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s <config.json> <base dir> THRESHOLD MAX_ABOVE MIN STEP <out>\n", argv[0]);
        return 2;
    }
    try {
        crt::TaskObjs all_objs;
        crt_task task = crt::load_task(argv[1], &all_objs);
        task.width = W; task.height = H; task.spp = S;
        crt::Scene scene(W, H);
        crt::load_task_scene(task, scene, argv[2], &all_objs);
        scene.set_BVH(task.bvh_thresh_n);
        crt_until_params up;
        ok(crt_until_defaults(&up), "crt_until_defaults");
        up.threshold = std::strtof(argv[3], nullptr); up.max_above = std::strtoull(argv[4], nullptr, 10);
        up.min_samples = (uint32_t)std::atoi(argv[5]); up.step_samples = (uint32_t)std::atoi(argv[6]);
        crt_camera cam;
        std::memcpy(cam.eye, task.eye_pos, sizeof(cam.eye));
        crt::get_inverse_view_matrix(task.eye_pos, task.lookat, task.up, cam.inv_view);
        cam.fov_y = task.fov_y * (float)M_PI / 180;
        crt_params p;
        std::memset(&p, 0, sizeof(p));
        p.width = W; p.height = H; p.spp = S; p.p_rr = task.p_rr; p.light_sample_n = (int32_t)task.light_sample_n;
        p.seed = 0; p.rank = 0; p.world = 1; p.traversal = CRT_TRAVERSAL_EXACT; p.flags = 0;
        crt_scene *direct = nullptr, *whole = nullptr;
        ok(crt_scene_create(&scene.flat(), 0, &direct), "crt_scene_create");
        ok(crt_scene_create(&scene.flat(), 0, &whole), "crt_scene_create");
        std::vector<uint8_t> rgb(3 * N);
        std::vector<float> mean(3 * N), var(3 * N);
        crt_until_info info;
        crt::Render r(&scene, S, task.p_rr, task.light_sample_n, 0);
        // the frame to the target
        ok(crt_render_until(direct, &cam, &p, &up, 0, rgb.data(), mean.data(), var.data(), &info), "crt_render_until");
        r.run_view_until(cam.eye, cam.inv_view, cam.fov_y, up, 0, true);
        same("run_view_until: frame", (const uint8_t*)r.get_frame_buffer(), rgb.data(), 3 * N);
        same("run_view_until: mean", r.get_mean_buffer(), mean.data(), 3 * N);
        same("run_view_until: variance", r.variance(), var.data(), 3 * N);
        same_info("run_view_until", r.last_until_info(), info);
        const uint32_t n = info.samples_done;
        crt_frame_error_info e;
        ok(crt_frame_error(direct, 0.07f, 0.02f, &e), "crt_frame_error");
        const crt_frame_error_info er = r.frame_error(0.07f, 0.02f);
        if (std::memcmp(&e, &er, sizeof(e)) != 0 || e.samples_done != n) fail("frame_error differs");
        std::FILE* f = std::fopen(argv[7], "wb");
        if (!f || std::fwrite(&n, sizeof(n), 1, f) != 1 || std::fwrite(rgb.data(), 1, 3 * N, f) != 3 * N || std::fwrite(mean.data(), sizeof(float), 3 * N, f) != 3 * N)
            fail(std::string("cannot write ") + argv[7]);
        std::fclose(f);
        // continued with a target nothing meets: to spp, and there the frame is crt_render's
        if (n < S) {
            up.threshold = 0.0f; up.max_above = 0;
            ok(crt_render_until(direct, &cam, &p, &up, n, rgb.data(), mean.data(), var.data(), &info), "crt_render_until, continued");
            r.run_view_until(cam.eye, cam.inv_view, cam.fov_y, up, n, false);
            same_info("run_view_until, continued", r.last_until_info(), info);
            if (info.samples_done != S) fail("threshold 0 stopped before spp");
            same("run_view_until, continued: frame", (const uint8_t*)r.get_frame_buffer(), rgb.data(), 3 * N);
            same("run_view_until, continued: mean", r.get_mean_buffer(), mean.data(), 3 * N);
            same("run_view_until, continued: variance", r.variance(), var.data(), 3 * N);
            p.flags = CRT_FLAG_VARIANCE;
            ok(crt_render(whole, &cam, &p, rgb.data(), mean.data(), nullptr), "crt_render");
            ok(crt_variance(whole, var.data(), nullptr), "crt_variance");
            same("run to spp: frame against crt_render", (const uint8_t*)r.get_frame_buffer(), rgb.data(), 3 * N);
            same("run to spp: mean against crt_render", r.get_mean_buffer(), mean.data(), 3 * N);
            same("run to spp: variance against crt_variance", r.variance(), var.data(), 3 * N);
        }
        crt_scene_destroy(direct);
        crt_scene_destroy(whole);
        std::printf("until_host_check: ok, %u samples\n", n);
    } catch (const crt::Error& e) {
        fail(std::string("unexpected error: ") + e.what() + " (" + crt_strerror(e.status) + ")");
    }
    return 0;
}
