// cudaraytracing_amd/csrc/crt_host_render.cpp -- crt::Render (see crt_host.hpp): the reference's Render class (include/Render.cuh:357-557)
// over the C ABI of include/crt.h.
#include "crt_host.hpp"

#include <algorithm>
#include <cstring>

namespace crt {

namespace {
// a library status as an Error: "`who` failed: ..." or, with the step of a longer method, "`who`: `step` failed: ..."
void check(int rc, std::string who, const char* step = nullptr)
{
    if (rc == CRT_OK) return;
    if (step) (who += ": ") += step;
    throw Error(rc, who + " failed: " + crt_last_error());
}
// what the save_* methods do once their buffer exists; `who` is the method's name
void save_rgb8(const char* who, const char* save_path, const Scene& scene, const std::vector<unsigned char>& rgb)
{
    check(crt_write_png(save_path, scene.get_width(), scene.get_height(), rgb.data()), who);
}
// a filter's settings at a frame size
template <class Params> Params sized(Params p, uint32_t w, uint32_t h)
{
    p.width = w; p.height = h;
    return p;
}
// one frame of a temporal sequence as the library takes it, and the buffers of the history it makes (Render::temporal_frame)
struct TemporalStep {
    crt_temporal_params p;
    crt_temporal_frame cur;
    const crt_temporal_history* prev;                    // nullptr: no history is continued
    std::vector<float> color, variance, history, m1, m2; // (m1, m2: of a history with moment planes)
    unsigned char* rgb;
};
} // namespace

// ------------------------------------------------------------------ Render --
// a Render that has given up its device objects runs nothing
void Render::alive(const char* who) const
{
    if (!device_scene_ && !multi_) throw Error(CRT_ERR_INVALID_ARG, std::string(who) + " after free()");
}
// every method but run_view works on one device only; `noun` is what the method's refusal calls it (nullptr: nothing)
void Render::one_device(const char* who, const char* noun) const
{
    if (multi_) throw Error(CRT_ERR_UNSUPPORTED, std::string(who) + ": " + (noun ? std::string(noun) + " is " : std::string()) + "a single-device interface");
    alive(who);
}
// the filters take the frame of run_view and the guides of run_aov
void Render::need_guides(const std::string& who) const
{
    const size_t n = scene_->get_pixels();
    if (albedo_buffer_.size() != 3 * n || normal_buffer_.size() != 3 * n || depth_buffer_.size() != n || mean_buffer_.size() != 3 * n)
        throw Error(CRT_ERR_INVALID_ARG, who + " needs run_view and run_aov of this frame size first");
}

Render::Render(Scene* scene, unsigned spp, float P_RR, unsigned light_sample_n, int device)
    : scene_(scene), spp_(spp), light_sample_n_(light_sample_n), P_RR_(P_RR), device_(device)
{
    if (!scene) throw Error(CRT_ERR_INVALID_ARG, "Render: null scene");
    const crt_scene_desc& d = scene->flat();
    check(crt_scene_create(&d, device, &device_scene_), "Render: crt_scene_create");
    frame_buffer_.assign((size_t)3 * scene->get_pixels(), 0);
    mean_buffer_.assign((size_t)3 * scene->get_pixels(), 0.0f);
}
// Several devices (the reference stops at device 0, src/main.cu:92-105): one replica of the scene per entry of `devices`, the
// frame sharded by interleaved pixel tiles and gathered with one RCCL all-gather (include/crt.h, crt_multi).
Render::Render(Scene* scene, unsigned spp, float P_RR, unsigned light_sample_n, const std::vector<int>& devices, uint32_t gather)
    : scene_(scene), spp_(spp), light_sample_n_(light_sample_n), P_RR_(P_RR)
{
    if (!scene) throw Error(CRT_ERR_INVALID_ARG, "Render: null scene");
    if (devices.empty()) throw Error(CRT_ERR_INVALID_ARG, "Render: empty device list");
    const crt_scene_desc& d = scene->flat();
    check(crt_multi_create(&d, devices.data(), (uint32_t)devices.size(), gather, &multi_), "Render: crt_multi_create");
    rank_stats_.resize(devices.size());
    frame_buffer_.assign((size_t)3 * scene->get_pixels(), 0);
    mean_buffer_.assign((size_t)3 * scene->get_pixels(), 0.0f);
}
Render::~Render() { free(); }

void Render::free()
{
    if (device_scene_) { crt_scene_destroy(device_scene_); device_scene_ = nullptr; }
    if (multi_) { crt_multi_destroy(multi_); multi_ = nullptr; }
}
void Render::set_denoise_scales(unsigned n)
{
    if (n < 1 || n > 4) throw Error(CRT_ERR_INVALID_ARG, "Render::set_denoise_scales: 1 .. 4 scales");
    denoise_scales_ = n;
}
void Render::set_width(const unsigned& w)
{
    scene_->set_width(w);
    frame_buffer_.assign((size_t)3 * scene_->get_pixels(), 0);
    mean_buffer_.assign((size_t)3 * scene_->get_pixels(), 0.0f);
}
void Render::set_height(const unsigned& h)
{
    scene_->set_height(h);
    frame_buffer_.assign((size_t)3 * scene_->get_pixels(), 0);
    mean_buffer_.assign((size_t)3 * scene_->get_pixels(), 0.0f);
}

// the camera and the settings of this object as the C ABI takes them: the whole frame on one rank, with the caller's flags
void Render::view_args(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t flags, crt_camera& cam, crt_params& p) const
{
    std::memcpy(cam.eye, eye_pos, sizeof(cam.eye));
    std::memcpy(cam.inv_view, inv_view_mat, sizeof(cam.inv_view));
    cam.fov_y = fovY;
    std::memset(&p, 0, sizeof(p));
    p.width = scene_->get_width(); p.height = scene_->get_height();
    p.spp = spp_; p.p_rr = P_RR_; p.light_sample_n = (int32_t)light_sample_n_;
    p.seed = seed_; p.rank = 0; p.world = 1; p.traversal = traversal_; p.flags = flags;
}

void Render::run_view(const float eye_pos[3], const float inv_view_mat[9], float fovY)
{
    alive("Render::run_view");
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, flags_ & (CRT_FLAG_TRACE_ALL | CRT_FLAG_BOUNDED_RADIANCE | CRT_FLAG_VARIANCE | CRT_FLAG_HALF_BUFFERS | CRT_FLAG_PIXEL_FILTER), cam, p);
    variance_buffer_.clear();
    int rc;
    if (multi_) {
        gathered_ = 0;
        rc = crt_multi_render(multi_, &cam, &p, frame_buffer_.data(), mean_buffer_.data(), rank_stats_.data(), &multi_info_);
        if (rc == CRT_OK) sum_rank_stats();
    } else rc = crt_render(device_scene_, &cam, &p, frame_buffer_.data(), mean_buffer_.data(), &stats_);
    check(rc, "Render::run_view");
}
// totals over the ranks; times of the slowest one
void Render::sum_rank_stats()
{
    stats_ = rank_stats_[0];
    for (size_t r = 1; r < rank_stats_.size(); r++) {
        const crt_stats& o = rank_stats_[r];
        stats_.paths += o.paths; stats_.rays += o.rays; stats_.shadow_rays += o.shadow_rays; stats_.probe_rays += o.probe_rays;
        stats_.rays_untraced += o.rays_untraced;
        stats_.kernel_ms = std::max(stats_.kernel_ms, o.kernel_ms); stats_.total_ms = std::max(stats_.total_ms, o.total_ms);
    }
}

// The frame of run_view with more of its buffers, gathered from all ranks (crt_multi_render_buffers): frame and mean buffers as run_view
// leaves them, every other plane of `want` in the buffer its single-device call fills here.
void Render::run_view_gathered(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t want)
{
    alive("Render::run_view_gathered");
    if (!multi_) throw Error(CRT_ERR_UNSUPPORTED, "Render::run_view_gathered gathers the buffers of a multi-device Render: on one device run_view, variance and run_aov make them");
    if (want & ~(uint32_t)CRT_MULTI_ALL) throw Error(CRT_ERR_INVALID_ARG, "Render::run_view_gathered: want holds a bit that is no CRT_MULTI_* plane");
    want |= CRT_MULTI_RGB | CRT_MULTI_MEAN;
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, flags_ & (CRT_FLAG_TRACE_ALL | CRT_FLAG_BOUNDED_RADIANCE), cam, p);
    const size_t n = scene_->get_pixels();
    gathered_ = 0;
    auto plane = [&](uint32_t bit, auto& v, size_t per_pixel) {
        if (want & bit) v.assign(per_pixel * n, 0); else v.clear();
        return (want & bit) ? v.data() : nullptr;
    };
    crt_multi_buffers out{};
    out.rgb = frame_buffer_.data(); out.mean = mean_buffer_.data();
    out.variance = plane(CRT_MULTI_VARIANCE, variance_buffer_, 3);
    out.half_a = plane(CRT_MULTI_HALF_A, half_a_buffer_, 3); out.half_b = plane(CRT_MULTI_HALF_B, half_b_buffer_, 3);
    out.albedo = plane(CRT_MULTI_ALBEDO, albedo_buffer_, 3); out.normal = plane(CRT_MULTI_NORMAL, normal_buffer_, 3);
    out.depth = plane(CRT_MULTI_DEPTH, depth_buffer_, 1); out.coverage = plane(CRT_MULTI_COVERAGE, coverage_buffer_, 1);
    out.tri = plane(CRT_MULTI_TRI, tri_buffer_, 1); out.material = plane(CRT_MULTI_MATERIAL, material_buffer_, 1);
    out.emission = plane(CRT_MULTI_EMISSION, emission_buffer_, 3); out.diffuse_albedo = plane(CRT_MULTI_DIFFUSE_ALBEDO, diffuse_albedo_buffer_, 3);
    check(crt_multi_render_buffers(multi_, &cam, &p, want, &out, rank_stats_.data(), &multi_info_), "Render::run_view_gathered");
    sum_rank_stats();
    gathered_ = want;
}
const void* Render::get_gathered_buffer(uint32_t plane) const
{
    if (!(gathered_ & plane)) return nullptr;
    switch (plane) {
    case CRT_MULTI_RGB: return frame_buffer_.data();
    case CRT_MULTI_MEAN: return mean_buffer_.data();
    case CRT_MULTI_VARIANCE: return variance_buffer_.data();
    case CRT_MULTI_HALF_A: return half_a_buffer_.data();
    case CRT_MULTI_HALF_B: return half_b_buffer_.data();
    case CRT_MULTI_ALBEDO: return albedo_buffer_.data();
    case CRT_MULTI_NORMAL: return normal_buffer_.data();
    case CRT_MULTI_DEPTH: return depth_buffer_.data();
    case CRT_MULTI_COVERAGE: return coverage_buffer_.data();
    case CRT_MULTI_TRI: return tri_buffer_.data();
    case CRT_MULTI_MATERIAL: return material_buffer_.data();
    case CRT_MULTI_EMISSION: return emission_buffer_.data();
    case CRT_MULTI_DIFFUSE_ALBEDO: return diffuse_albedo_buffer_.data();
    default: return nullptr;
    }
}

// the arguments and buffers run_view_adaptive, run_view_map and run_view_planned share: `render` makes the library call on them
template <class Call> void Render::sampled_frame(const char* who, const float eye_pos[3], const float inv_view_mat[9], float fovY, bool want_variance, Call render)
{
    one_device(who, nullptr);
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, flags_ & CRT_FLAG_TRACE_ALL, cam, p);
    const size_t n = scene_->get_pixels();
    samples_buffer_.assign(n, 0u);
    variance_buffer_.clear();
    std::vector<float> v(want_variance ? 3 * n : 0, 0.0f);
    check(render(&cam, &p, want_variance ? v.data() : nullptr), who);
    variance_buffer_.swap(v);
}

void Render::run_view_adaptive(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_adaptive_params& ap, bool want_variance)
{
    sampled_frame("Render::run_view_adaptive", eye_pos, inv_view_mat, fovY, want_variance, [&](const crt_camera* cam, const crt_params* p, float* var) {
        return crt_render_adaptive(device_scene_, cam, p, &ap, frame_buffer_.data(), mean_buffer_.data(), samples_buffer_.data(), var, &adaptive_info_);
    });
}

void Render::run_view_map(const float eye_pos[3], const float inv_view_mat[9], float fovY, const uint32_t* sample_map, uint32_t sample_begin, bool want_variance)
{
    sampled_frame("Render::run_view_map", eye_pos, inv_view_mat, fovY, want_variance, [&](const crt_camera* cam, const crt_params* p, float* var) {
        return crt_render_map(device_scene_, cam, p, sample_map, sample_begin, frame_buffer_.data(), mean_buffer_.data(), samples_buffer_.data(), var, &map_info_);
    });
}

void Render::run_view_planned(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_adaptive_params& ap, bool want_variance)
{
    sampled_frame("Render::run_view_planned", eye_pos, inv_view_mat, fovY, want_variance, [&](const crt_camera* cam, const crt_params* p, float* var) {
        return crt_render_planned(device_scene_, cam, p, &ap, frame_buffer_.data(), mean_buffer_.data(), samples_buffer_.data(), var, &map_info_);
    });
}

crt_refit_info Render::refit()
{
    one_device("Render::refit", "a refit of the scene handle");
    const crt_scene_desc& d = scene_->flat();
    crt_refit_info r{};
    check(crt_scene_refit(device_scene_, d.tris, d.n_tris, d.light_tris, d.n_light_tris, &r), "Render::refit");
    return r;
}

crt_frame_error_info Render::frame_error(float threshold, float mean_floor)
{
    one_device("Render::frame_error", "the frame's error summary");
    crt_frame_error_info e{};
    check(crt_frame_error(device_scene_, threshold, mean_floor, &e), "Render::frame_error");
    return e;
}

void Render::run_view_until(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_until_params& up, uint32_t sample_begin, bool want_variance)
{
    one_device("Render::run_view_until", "rendering to an error target");
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, flags_ & CRT_FLAG_TRACE_ALL, cam, p);
    variance_buffer_.clear();
    std::vector<float> v(want_variance ? 3 * scene_->get_pixels() : 0, 0.0f);
    check(crt_render_until(device_scene_, &cam, &p, &up, sample_begin, frame_buffer_.data(), mean_buffer_.data(), want_variance ? v.data() : nullptr, &until_info_),
          "Render::run_view_until");
    variance_buffer_.swap(v);
}

void Render::run_aov(const float eye_pos[3], const float inv_view_mat[9], float fovY)
{
    one_device("Render::run_aov", "the AOV pass");
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, 0, cam, p);
    const size_t n = scene_->get_pixels();
    albedo_buffer_.assign(3 * n, 0.0f); normal_buffer_.assign(3 * n, 0.0f); depth_buffer_.assign(n, 0.0f); material_buffer_.assign(n, 0);
    crt_aov_buffers out{};
    out.albedo = albedo_buffer_.data(); out.normal = normal_buffer_.data(); out.depth = depth_buffer_.data(); out.material = material_buffer_.data();
    int rc;
    if (aov_shading_) {
        emission_buffer_.assign(3 * n, 0.0f); diffuse_albedo_buffer_.assign(3 * n, 0.0f);
        const crt_aov_shading_buffers shading{emission_buffer_.data(), diffuse_albedo_buffer_.data()};
        rc = crt_render_aov_shading(device_scene_, &cam, &p, &out, &shading, &aov_info_);
    } else rc = crt_render_aov(device_scene_, &cam, &p, &out, &aov_info_);
    check(rc, "Render::run_aov");
}

void Render::run_view_aov_direct(const float eye_pos[3], const float inv_view_mat[9], float fovY)
{
    one_device("Render::run_view_aov_direct", "the AOV pass");
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, 0, cam, p);
    const size_t n = scene_->get_pixels();
    direct_buffer_.assign(3 * n, 0.0f); unshadowed_buffer_.assign(3 * n, 0.0f); direct_variance_buffer_.assign(3 * n, 0.0f); visibility_buffer_.assign(n, 0.0f);
    const crt_aov_direct_buffers out{direct_buffer_.data(), unshadowed_buffer_.data(), direct_variance_buffer_.data(), visibility_buffer_.data()};
    check(crt_render_aov_direct(device_scene_, &cam, &p, &out, &aov_direct_info_), "Render::run_view_aov_direct");
}

void Render::run_view_aov_ao(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t ao_samples, float max_distance)
{
    one_device("Render::run_view_aov_ao", "the AOV pass");
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, 0, cam, p);
    crt_aov_ao_params ao;
    check(crt_aov_ao_defaults(device_scene_, &ao), "Render::run_view_aov_ao");
    if (ao_samples != 0) ao.ao_samples = ao_samples;
    if (max_distance != 0.0f) ao.max_distance = max_distance;
    const size_t n = scene_->get_pixels();
    ao_buffer_.assign(n, 0.0f); openness_buffer_.assign(n, 0.0f); bent_normal_buffer_.assign(3 * n, 0.0f);
    const crt_aov_ao_buffers out{ao_buffer_.data(), openness_buffer_.data(), bent_normal_buffer_.data()};
    check(crt_render_aov_ao(device_scene_, &cam, &p, &ao, &out, &aov_ao_info_), "Render::run_view_aov_ao");
}

crt_modulate_params Render::modulate_params(const char* who) const
{
    if (emission_buffer_.size() != (size_t)3 * scene_->get_pixels() || diffuse_albedo_buffer_.size() != emission_buffer_.size())
        throw Error(CRT_ERR_INVALID_ARG, std::string(who) + " with set_demodulate needs run_aov of this frame size first");
    crt_modulate_params m;
    crt_modulate_defaults(&m);
    m.width = scene_->get_width(); m.height = scene_->get_height(); m.albedo_floor = albedo_floor_;
    return m;
}

// crt_demodulate of a colour (and its variance, if any) with the shading AOVs of the last run_aov
void Render::demodulate_of(const char* who, const float* color, const float* variance, std::vector<float>& irradiance, std::vector<float>& irradiance_variance) const
{
    const crt_modulate_params m = modulate_params(who);
    const size_t n = scene_->get_pixels();
    irradiance.assign(3 * n, 0.0f);
    if (variance) irradiance_variance.assign(3 * n, 0.0f);
    check(crt_demodulate(device_, &m, color, diffuse_albedo_buffer_.data(), emission_buffer_.data(), variance, irradiance.data(),
                         variance ? irradiance_variance.data() : nullptr, nullptr), who);
}

// crt_modulate of an irradiance with the same buffers
void Render::modulate_of(const char* who, const float* irradiance, float* out_mean, unsigned char* out_rgb) const
{
    const crt_modulate_params m = modulate_params(who);
    check(crt_modulate(device_, &m, irradiance, diffuse_albedo_buffer_.data(), emission_buffer_.data(), out_mean, out_rgb, nullptr), who);
}

void Render::run_aov_specular(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t max_bounces, bool as_albedo_guide)
{
    one_device("Render::run_aov_specular", "the AOV pass");
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, 0, cam, p);
    crt_aov_specular_params sp;
    crt_aov_specular_defaults(&sp);
    if (max_bounces) sp.max_bounces = max_bounces;
    const size_t n = scene_->get_pixels();
    guide_albedo_buffer_.assign(3 * n, 0.0f); last_normal_buffer_.assign(3 * n, 0.0f); path_depth_buffer_.assign(n, 0.0f); bounces_buffer_.assign(n, 0.0f);
    crt_aov_specular_buffers out{};
    out.guide_albedo = guide_albedo_buffer_.data(); out.last_normal = last_normal_buffer_.data(); out.path_depth = path_depth_buffer_.data();
    out.bounces = bounces_buffer_.data();
    check(crt_render_aov_specular(device_scene_, &cam, &p, &sp, &out, &aov_specular_info_), "Render::run_aov_specular");
    if (as_albedo_guide) albedo_buffer_ = guide_albedo_buffer_;
}

const float* Render::variance()
{
    one_device("Render::variance", "the variance buffer");
    if (variance_buffer_.empty()) {
        std::vector<float> v(3 * scene_->get_pixels(), 0.0f);
        check(crt_variance(device_scene_, v.data(), nullptr), "Render::variance");
        variance_buffer_.swap(v);
    }
    return variance_buffer_.data();
}

void Render::set_pixel_filter(const crt_pixel_filter* filter)
{
    one_device("Render::set_pixel_filter", "the pixel filter");
    check(crt_set_pixel_filter(device_scene_, filter), "Render::set_pixel_filter");
}
void Render::filtered_frame()
{
    one_device("Render::filtered_frame", "the filtered frame");
    std::vector<unsigned char> rgb(3 * scene_->get_pixels(), 0);
    std::vector<float> mean(3 * scene_->get_pixels(), 0.0f);
    check(crt_filtered_frame(device_scene_, rgb.data(), mean.data(), nullptr), "Render::filtered_frame");
    filtered_buffer_.swap(rgb); filtered_mean_buffer_.swap(mean);
}

Render::Filter Render::default_filter(int kind)
{
    Filter f{kind};
    if (kind == SELECT_VAR) crt_denoise_var_defaults(&f.dn); else crt_denoise_defaults(&f.dn);
    crt_denoise_nlm_defaults(&f.nlm); crt_denoise_regress_defaults(&f.reg);
    return f;
}

// The library call of `f` on the planes `l` of a w x h frame, with f's settings at that size: the one place that knows how the four
// calls differ.  The caller's pointers go to the library as they are.  weights: the image the regression filter takes its weights
// from, with l.variance as its variance (nullptr: the frame's own).  Returns the status.  info may be null; the regression filter has
// an info of its own, which with an `info` goes to regress_info_ and gives `info` its timer and its one pass.
int Render::apply_filter(const Filter& f, uint32_t w, uint32_t h, const crt_pyramid_planes& l, const float* weights, float* out_mean, unsigned char* out_rgb,
                         crt_denoise_info* info)
{
    if (f.kind == SELECT_ATROUS) {
        const crt_denoise_params p = sized(f.dn, w, h);
        const crt_denoise_inputs in{l.color, l.albedo, l.normal, l.depth};
        return crt_denoise(device_, &p, &in, out_mean, out_rgb, info);
    }
    if (f.kind == SELECT_REG) {
        const crt_regress_params p = sized(f.reg, w, h);
        const crt_regress_inputs in{l.color, l.variance, weights, weights ? l.variance : nullptr, l.albedo, l.normal, l.depth};
        const int rc = crt_denoise_regress(device_, &p, &in, out_mean, out_rgb, info ? &regress_info_ : nullptr);
        if (info) { info->total_ms = regress_info_.total_ms; info->passes = 1; }
        return rc;
    }
    const crt_denoise_var_inputs in{l.color, l.variance, l.albedo, l.normal, l.depth};
    if (f.kind == SELECT_NLM) {
        const crt_nlm_params p = sized(f.nlm, w, h);
        return crt_denoise_nlm(device_, &p, &in, out_mean, out_rgb, nullptr, info);
    }
    const crt_denoise_params p = sized(f.dn, w, h);
    return crt_denoise_var(device_, &p, &in, out_mean, out_rgb, nullptr, info);
}

// `f` once per scale of a Laplacian pyramid of `scales` scales over the planes `in` of a w x h frame, from the coarsest scale up
// (crt_pyramid_down, crt_pyramid_merge: the chain of denoise_multiscale in api.py); scales 1: the one call.  denoise_info_ holds the sum
// of every call's timer and of the filter's passes afterwards, regress_info_ the finest scale's call, which is the last.
void Render::filter_scales(const char* who, const Filter& f, unsigned scales, uint32_t w, uint32_t h, const crt_pyramid_planes& in, float* out_mean, unsigned char* out_rgb)
{
    if (scales <= 1) {
        check(apply_filter(f, w, h, in, nullptr, out_mean, out_rgb, &denoise_info_), who);
        return;
    }
    struct Level {
        uint32_t w, h;
        std::vector<float> color, variance, albedo, normal, depth;
        crt_pyramid_planes planes;
    };
    std::vector<Level> levels(scales); // level 0: the caller's planes
    levels[0].w = w; levels[0].h = h; levels[0].planes = in;
    float total_ms = 0.0f;
    uint32_t passes = 0;
    crt_pyramid_info pinfo{};
    for (unsigned k = 1; k < scales; k++) {
        const Level& fine = levels[k - 1];
        Level& c = levels[k];
        crt_pyramid_params pp{fine.w, fine.h, (fine.w + 1) / 2, (fine.h + 1) / 2};
        c.w = pp.low_width; c.h = pp.low_height;
        const size_t n = (size_t)c.w * c.h;
        c.color.assign(3 * n, 0.0f);
        if (fine.planes.variance) c.variance.assign(3 * n, 0.0f);
        if (fine.planes.albedo) c.albedo.assign(3 * n, 0.0f);
        if (fine.planes.normal) c.normal.assign(3 * n, 0.0f);
        if (fine.planes.depth) c.depth.assign(n, 0.0f);
        auto ptr = [](std::vector<float>& v) { return v.empty() ? nullptr : v.data(); };
        crt_pyramid_out_planes out{ptr(c.color), ptr(c.variance), ptr(c.albedo), ptr(c.normal), ptr(c.depth)};
        check(crt_pyramid_down(device_, &pp, &fine.planes, &out, &pinfo), who);
        total_ms += pinfo.total_ms;
        c.planes = crt_pyramid_planes{out.color, out.variance, out.albedo, out.normal, out.depth};
    }
    std::vector<float> result, filtered, merged;
    for (unsigned k = scales; k-- > 0;) {
        const Level& l = levels[k];
        const size_t n = (size_t)l.w * l.h;
        std::vector<float>& dst = k + 1 == scales ? result : filtered;
        dst.assign(3 * n, 0.0f);
        check(apply_filter(f, l.w, l.h, l.planes, nullptr, dst.data(), nullptr, &denoise_info_), who);
        total_ms += denoise_info_.total_ms; passes += denoise_info_.passes;
        if (k + 1 == scales) continue;
        crt_pyramid_params pp{l.w, l.h, (l.w + 1) / 2, (l.h + 1) / 2};
        if (k == 0) check(crt_pyramid_merge(device_, &pp, filtered.data(), result.data(), out_mean, out_rgb, &pinfo), who);
        else {
            merged.assign(3 * n, 0.0f);
            check(crt_pyramid_merge(device_, &pp, filtered.data(), result.data(), merged.data(), nullptr, &pinfo), who);
            result.swap(merged);
        }
        total_ms += pinfo.total_ms;
    }
    denoise_info_.total_ms = total_ms; denoise_info_.passes = passes;
}

// `f` of a colour and its variance (nullptr: a-trous takes none) with the guides of the last run_aov, at `scales` scales, into the
// denoised buffers.  set_demodulate: on irradiance -- the colour and variance are demodulated first unless they are irradiance already,
// the regression filter loses its albedo feature, which irradiance does not follow -- and modulated after: the filter then writes no
// RGB8, the tone map comes from crt_modulate.
void Render::denoise_of(const char* who, Filter f, const float* color, const float* variance, bool is_irradiance, unsigned scales)
{
    const size_t n = scene_->get_pixels();
    std::vector<float> irradiance, irradiance_variance;
    if (demodulate_ && !is_irradiance) {
        demodulate_of(who, color, variance, irradiance, irradiance_variance);
        color = irradiance.data();
        if (variance) variance = irradiance_variance.data();
    }
    if (demodulate_ && f.kind == SELECT_REG) f.reg.features &= ~CRT_REGRESS_ALBEDO;
    const crt_pyramid_planes planes{color, variance, albedo_buffer_.data(), normal_buffer_.data(), depth_buffer_.data()};
    denoised_buffer_.assign(3 * n, 0); denoised_mean_buffer_.assign(3 * n, 0.0f);
    filter_scales(who, f, scales, scene_->get_width(), scene_->get_height(), planes, denoised_mean_buffer_.data(), demodulate_ ? nullptr : denoised_buffer_.data());
    if (demodulate_) modulate_of(who, denoised_mean_buffer_.data(), denoised_mean_buffer_.data(), denoised_buffer_.data());
}

// the frame of the last run_view through one filter.  (run_denoise has one scale whatever set_denoise_scales says: no variance to reduce)
void Render::run_denoise(const crt_denoise_params& prm)
{
    one_device("Render::run_denoise", "the denoiser");
    need_guides("Render::run_denoise");
    denoise_of("Render::run_denoise", Filter{SELECT_ATROUS, prm}, mean_buffer_.data(), nullptr, false, 1);
}

void Render::run_denoise_var(const crt_denoise_params& prm)
{
    one_device("Render::run_denoise_var", "the denoiser");
    need_guides("Render::run_denoise_var");
    denoise_of("Render::run_denoise_var", Filter{SELECT_VAR, prm}, mean_buffer_.data(), variance(), false, denoise_scales_);
}

void Render::run_denoise_nlm(const crt_nlm_params& prm)
{
    one_device("Render::run_denoise_nlm", "the denoiser");
    need_guides("Render::run_denoise_nlm");
    denoise_of("Render::run_denoise_nlm", Filter{SELECT_NLM, {}, prm}, mean_buffer_.data(), variance(), false, denoise_scales_);
}

void Render::run_denoise_regress(const crt_regress_params& prm)
{
    one_device("Render::run_denoise_regress", "the denoiser");
    need_guides("Render::run_denoise_regress");
    denoise_of("Render::run_denoise_regress", Filter{SELECT_REG, {}, {}, prm}, mean_buffer_.data(), variance(), false, denoise_scales_);
}

void Render::run_denoise_select(const std::vector<int>& candidates, const crt_filter_select_params& prm)
{
    const char* who = "Render::run_denoise_select";
    one_device(who, "filter selection");
    if (demodulate_) throw Error(CRT_ERR_UNSUPPORTED, std::string(who) + ": the half frames are filtered as radiance (not with set_demodulate)");
    if (candidates.empty() || candidates.size() > CRT_SELECT_MAX_CANDIDATES) throw Error(CRT_ERR_INVALID_ARG, std::string(who) + " needs 1 .. 4 candidates");
    const size_t n = scene_->get_pixels();
    need_guides(who);
    std::vector<float> half[2] = {std::vector<float>(3 * n), std::vector<float>(3 * n)}, half_variance(3 * n);
    check(crt_half_buffers(device_scene_, half[0].data(), half[1].data(), nullptr), who);
    const float* var = variance();
    for (size_t i = 0; i < 3 * n; i++) half_variance[i] = 2.0f * var[i];
    const uint32_t w = scene_->get_width(), h = scene_->get_height();
    std::vector<std::vector<float>> filtered[2];
    crt_filter_select_inputs in{};
    in.half_a = half[0].data(); in.half_b = half[1].data(); in.half_variance = half_variance.data();
    for (int side = 0; side < 2; side++) {
        filtered[side].resize(candidates.size());
        for (size_t k = 0; k < candidates.size(); k++) {
            const float* image = half[side].data();
            if (candidates[k] != SELECT_NONE) { // the filter with its own defaults and the guides of the last run_aov; weights from the other half
                if (candidates[k] < SELECT_ATROUS || candidates[k] > SELECT_REG) throw Error(CRT_ERR_INVALID_ARG, std::string(who) + ": unknown candidate");
                filtered[side][k].assign(3 * n, 0.0f);
                const crt_pyramid_planes planes{image, half_variance.data(), albedo_buffer_.data(), normal_buffer_.data(), depth_buffer_.data()};
                check(apply_filter(default_filter(candidates[k]), w, h, planes, half[1 - side].data(), filtered[side][k].data(), nullptr, nullptr), who);
                image = filtered[side][k].data();
            }
            (side == 0 ? in.filtered_a : in.filtered_b)[k] = image;
        }
    }
    crt_filter_select_params p = prm;
    p.width = w; p.height = h; p.n_candidates = (uint32_t)candidates.size();
    denoised_buffer_.assign(3 * n, 0); denoised_mean_buffer_.assign(3 * n, 0.0f); choice_buffer_.assign(n, 0);
    check(crt_filter_select(device_, &p, &in, denoised_mean_buffer_.data(), denoised_buffer_.data(), choice_buffer_.data(), nullptr, &select_info_), who);
}

// What run_temporal, run_temporal_specular and run_temporal_moments share, around the library calls `blend` makes on the step.  Before them:
// the size and the cameras, whether the history is continued (one with moment planes or with specular planes is not continued without them,
// nor the other way round; `specular`: the step keeps the planes run_aov_specular has just written with the history), the frame
// with `var`, the variance of its mean (nullptr: none is carried), or its irradiance, and the history.  After them: a failure drops the
// history; otherwise the step's buffers become it, with the frame's guides, camera and size.
template <class Blend> void Render::temporal_frame(const char* who, const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm,
                                                   bool moments, const float* var, Blend blend, bool specular)
{
    TemporalStep s{};
    s.p = prm;
    s.p.width = scene_->get_width(); s.p.height = scene_->get_height();
    std::memcpy(s.p.cur.eye, eye_pos, sizeof(s.p.cur.eye));
    std::memcpy(s.p.cur.inv_view, inv_view_mat, sizeof(s.p.cur.inv_view));
    s.p.cur.fov_y = fovY;
    const bool have = temporal_valid_ && temporal_moments_ == moments && temporal_specular_ == specular && temporal_demodulated_ == demodulate_ &&
                      temporal_width_ == s.p.width && temporal_height_ == s.p.height;
    s.p.prev = have ? temporal_cam_ : s.p.cur;
    const size_t n = scene_->get_pixels();
    s.cur.color = mean_buffer_.data(); s.cur.variance = var; s.cur.depth = depth_buffer_.data(); s.cur.normal = normal_buffer_.data(); s.cur.id = material_buffer_.data();
    std::vector<float> irradiance, irradiance_variance;
    if (demodulate_) {
        demodulate_of(who, mean_buffer_.data(), var, irradiance, irradiance_variance);
        s.cur.color = irradiance.data();
        if (var) s.cur.variance = irradiance_variance.data();
    }
    crt_temporal_history prev{};
    prev.color = temporal_color_.data(); prev.variance = moments ? nullptr : temporal_variance_.data(); prev.history = temporal_history_.data();
    prev.depth = temporal_depth_.data(); prev.normal = temporal_normal_.data(); prev.id = temporal_id_.data();
    s.prev = have ? &prev : nullptr;
    s.color.assign(3 * n, 0.0f); s.variance.assign(3 * n, 0.0f); s.history.assign(n, 0.0f);
    if (moments) { s.m1.assign(3 * n, 0.0f); s.m2.assign(3 * n, 0.0f); }
    temporal_rgb_.assign(3 * n, 0);
    s.rgb = demodulate_ ? nullptr : temporal_rgb_.data(); // (irradiance has no tone map worth having: modulate_of writes the RGB8 below)
    const int rc = blend(s);
    if (rc != CRT_OK) temporal_valid_ = false;
    check(rc, who);
    if (demodulate_) modulate_of(who, s.color.data(), nullptr, temporal_rgb_.data());
    temporal_demodulated_ = demodulate_;
    temporal_color_.swap(s.color); temporal_variance_.swap(s.variance); temporal_history_.swap(s.history);
    if (moments) { temporal_m1_.swap(s.m1); temporal_m2_.swap(s.m2); }
    temporal_depth_ = depth_buffer_; temporal_normal_ = normal_buffer_; temporal_id_ = material_buffer_;
    if (specular) { temporal_path_depth_ = path_depth_buffer_; temporal_bounces_ = bounces_buffer_; temporal_last_normal_ = last_normal_buffer_; }
    temporal_specular_ = specular;
    temporal_cam_ = s.p.cur; temporal_width_ = s.p.width; temporal_height_ = s.p.height;
    temporal_valid_ = true;
    temporal_moments_ = moments;
}

void Render::run_temporal(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm, const crt_temporal_clamp* clamp)
{
    const char* who = "Render::run_temporal";
    one_device(who, "temporal accumulation");
    if (!(flags_ & CRT_FLAG_VARIANCE)) throw Error(CRT_ERR_INVALID_ARG, std::string(who) + " needs set_flags(CRT_FLAG_VARIANCE)");
    run_view(eye_pos, inv_view_mat, fovY);
    const float* var = variance();
    run_aov(eye_pos, inv_view_mat, fovY);
    temporal_frame(who, eye_pos, inv_view_mat, fovY, prm, false, var, [&](TemporalStep& s) {
        temporal_clamped_ = 0;
        if (!clamp) return crt_temporal(device_, &s.p, &s.cur, s.prev, s.color.data(), s.variance.data(), s.history.data(), s.rgb, &temporal_info_);
        crt_temporal_clamp_info ci{};
        const int rc = crt_temporal_clamped(device_, &s.p, clamp, &s.cur, s.prev, s.color.data(), s.variance.data(), s.history.data(), s.rgb, &ci);
        temporal_info_.total_ms = ci.total_ms; temporal_info_.reprojected = ci.reprojected;
        temporal_clamped_ = ci.clamped;
        return rc;
    }, false);
}

void Render::run_temporal_specular(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm, const crt_temporal_clamp* clamp,
                                   const crt_temporal_dual_params& dual, uint32_t max_bounces)
{
    const char* who = "Render::run_temporal_specular";
    one_device(who, "temporal accumulation");
    if (!(flags_ & CRT_FLAG_VARIANCE)) throw Error(CRT_ERR_INVALID_ARG, std::string(who) + " needs set_flags(CRT_FLAG_VARIANCE)");
    run_view(eye_pos, inv_view_mat, fovY);
    const float* var = variance();
    run_aov(eye_pos, inv_view_mat, fovY);
    run_aov_specular(eye_pos, inv_view_mat, fovY, max_bounces, false);
    temporal_frame(who, eye_pos, inv_view_mat, fovY, prm, false, var, [&](TemporalStep& s) {
        const crt_temporal_specular_planes cur_spec = {path_depth_buffer_.data(), bounces_buffer_.data(), last_normal_buffer_.data()};
        const crt_temporal_specular_planes prev_spec = {temporal_path_depth_.data(), temporal_bounces_.data(), temporal_last_normal_.data()};
        const int rc = crt_temporal_dual(device_, &s.p, clamp, &dual, &s.cur, &cur_spec, s.prev, s.prev ? &prev_spec : nullptr, s.color.data(), s.variance.data(),
                                         s.history.data(), s.rgb, &temporal_dual_info_);
        temporal_info_.total_ms = temporal_dual_info_.total_ms; temporal_info_.reprojected = temporal_dual_info_.reprojected;
        temporal_clamped_ = temporal_dual_info_.clamped;
        return rc;
    }, true);
}

void Render::run_temporal_moments(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm, const crt_temporal_clamp* clamp,
                                  const crt_variance_estimate_params& est)
{
    const char* who = "Render::run_temporal_moments";
    one_device(who, "temporal accumulation");
    run_view(eye_pos, inv_view_mat, fovY);
    run_aov(eye_pos, inv_view_mat, fovY);
    temporal_frame(who, eye_pos, inv_view_mat, fovY, prm, true, nullptr, [&](TemporalStep& s) {
        const crt_temporal_moment_planes planes = {temporal_m1_.data(), temporal_m2_.data()};
        crt_temporal_clamp_info ci{};
        const int rc = crt_temporal_moments(device_, &s.p, clamp, &s.cur, s.prev, s.prev ? &planes : nullptr, s.color.data(), nullptr, s.history.data(), s.m1.data(),
                                            s.m2.data(), s.rgb, &ci);
        if (rc != CRT_OK) return rc;
        temporal_info_.total_ms = ci.total_ms; temporal_info_.reprojected = ci.reprojected;
        temporal_clamped_ = ci.clamped;
        crt_variance_estimate_params e = est; // the variance the history keeps: the estimate from its moments
        e.width = s.p.width; e.height = s.p.height;
        crt_variance_estimate_inputs in{};
        in.m1 = s.m1.data(); in.m2 = s.m2.data(); in.history = s.history.data(); in.normal = normal_buffer_.data(); in.depth = depth_buffer_.data();
        return crt_variance_estimate(device_, &e, &in, s.variance.data(), &estimate_info_);
    }, false);
}

void Render::run_denoise_temporal(const crt_denoise_params& prm)
{
    if (!temporal_valid_ || temporal_color_.size() != (size_t)3 * scene_->get_pixels())
        throw Error(CRT_ERR_INVALID_ARG, "Render::run_denoise_temporal needs run_temporal of this frame size first");
    if (temporal_demodulated_ != demodulate_) throw Error(CRT_ERR_INVALID_ARG, "Render::run_denoise_temporal: set_demodulate changed since run_temporal");
    denoise_of("Render::run_denoise_temporal", Filter{SELECT_VAR, prm}, temporal_color_.data(), temporal_variance_.data(), temporal_demodulated_, 1);
}

void Render::run_view_upsampled(const float eye_pos[3], const float inv_view_mat[9], float fovY, unsigned factor, const crt_upsample_params& prm, unsigned guide_spp)
{
    const char* who = "Render::run_view_upsampled";
    one_device(who, "upsampling");
    const unsigned W = scene_->get_width(), H = scene_->get_height();
    if (factor < 2 || factor > 8) throw Error(CRT_ERR_INVALID_ARG, std::string(who) + ": the factor must be 2 .. 8");
    if (W % factor || H % factor) throw Error(CRT_ERR_INVALID_ARG, std::string(who) + ": the factor must divide width and height");
    const unsigned lw = W / factor, lh = H / factor;
    const size_t nl = (size_t)lw * lh, n = scene_->get_pixels();
    // the low-resolution frame, its variance and its AOVs
    crt_camera cam;
    crt_params p;
    view_args(eye_pos, inv_view_mat, fovY, (flags_ & (CRT_FLAG_TRACE_ALL | CRT_FLAG_BOUNDED_RADIANCE)) | CRT_FLAG_VARIANCE, cam, p);
    p.width = lw; p.height = lh;
    std::vector<unsigned char> low_rgb(3 * nl, 0);
    std::vector<float> low_mean(3 * nl, 0.0f), low_var(3 * nl, 0.0f), l_albedo(3 * nl, 0.0f), l_normal(3 * nl, 0.0f), l_depth(nl, 0.0f), l_emission(3 * nl, 0.0f),
        l_diffuse(3 * nl, 0.0f);
    crt_stats low_stats;
    variance_buffer_.clear(); // (the handle's sums are the low frame's from here on)
    check(crt_render(device_scene_, &cam, &p, low_rgb.data(), low_mean.data(), &low_stats), who, "the low-resolution frame");
    check(crt_variance(device_scene_, low_var.data(), nullptr), who, "its variance");
    p.flags = 0;
    crt_aov_buffers la{};
    la.albedo = l_albedo.data(); la.normal = l_normal.data(); la.depth = l_depth.data();
    const crt_aov_shading_buffers ls{l_emission.data(), l_diffuse.data()};
    crt_aov_info low_aov;
    check(crt_render_aov_shading(device_scene_, &cam, &p, &la, &ls, &low_aov), who, "the low-resolution AOV pass");
    {   // the full-resolution AOVs: run_aov with the shading buffers and guide_spp samples; the settings come back however it ends
        struct Restore { bool& shading; unsigned& spp; const bool shading_was; const unsigned spp_was; ~Restore() { shading = shading_was; spp = spp_was; } }
            restore{aov_shading_, spp_, aov_shading_, spp_};
        aov_shading_ = true;
        if (guide_spp) spp_ = guide_spp;
        run_aov(eye_pos, inv_view_mat, fovY);
    }
    // irradiance at the low size, upsampled, radiance at the full size
    crt_modulate_params m;
    crt_modulate_defaults(&m);
    m.width = lw; m.height = lh; m.albedo_floor = albedo_floor_;
    std::vector<float> irr(3 * nl, 0.0f), ivar(3 * nl, 0.0f), up(3 * n, 0.0f), up_var(3 * n, 0.0f);
    check(crt_demodulate(device_, &m, low_mean.data(), l_diffuse.data(), l_emission.data(), low_var.data(), irr.data(), ivar.data(), nullptr), who, "crt_demodulate");
    crt_upsample_params u = prm;
    u.width = W; u.height = H; u.low_width = lw; u.low_height = lh;
    const crt_upsample_low low{irr.data(), ivar.data(), l_albedo.data(), l_normal.data(), l_depth.data()};
    const crt_upsample_guides guides{albedo_buffer_.data(), normal_buffer_.data(), depth_buffer_.data()};
    check(crt_upsample(device_, &u, &low, &guides, up.data(), up_var.data(), nullptr, &upsample_info_), who, "crt_upsample");
    upsampled_buffer_.assign(3 * n, 0); upsampled_mean_buffer_.assign(3 * n, 0.0f);
    m.width = W; m.height = H;
    check(crt_modulate(device_, &m, up.data(), diffuse_albedo_buffer_.data(), emission_buffer_.data(), upsampled_mean_buffer_.data(), upsampled_buffer_.data(), nullptr),
          who, "crt_modulate");
}

void Render::save_upsampled_buffer(const char* save_path) const
{
    if (upsampled_buffer_.empty()) throw Error(CRT_ERR_INVALID_ARG, "save_upsampled_buffer before run_view_upsampled");
    save_rgb8("save_upsampled_buffer", save_path, *scene_, upsampled_buffer_);
}

void Render::save_temporal_buffer(const char* save_path) const
{
    if (temporal_rgb_.empty()) throw Error(CRT_ERR_INVALID_ARG, "save_temporal_buffer before run_temporal");
    save_rgb8("save_temporal_buffer", save_path, *scene_, temporal_rgb_);
}

void Render::save_denoised_buffer(const char* save_path) const
{
    if (denoised_buffer_.empty()) throw Error(CRT_ERR_INVALID_ARG, "save_denoised_buffer before run_denoise");
    save_rgb8("save_denoised_buffer", save_path, *scene_, denoised_buffer_);
}

void Render::save_filtered_buffer(const char* save_path) const
{
    if (filtered_buffer_.empty()) throw Error(CRT_ERR_INVALID_ARG, "save_filtered_buffer before filtered_frame");
    save_rgb8("save_filtered_buffer", save_path, *scene_, filtered_buffer_);
}

void Render::save_frame_buffer(const char* save_path) const { save_rgb8("save_frame_buffer", save_path, *scene_, frame_buffer_); }

} // namespace crt
