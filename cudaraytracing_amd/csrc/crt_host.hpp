// cudaraytracing_amd/csrc/crt_host.hpp
//
// Host side of the path tracer, above the C ABI of include/crt.h: the C++
// classes a user of the reference knows -- Material, Triangle, Object, BVH,
// Scene, Loader, Task, Render and get_inverse_view_matrix -- re-implemented
// for a flat, upload-ready data model (structure-of-arrays friendly PODs,
// de-duplicated material table, index-permutation BVH build).
//
// Same names, argument meaning and results as the reference classes
// (include/Scene.h, Object.h, Triangle.h, Material.h, BVH.h, Loader.h,
// OBJLoader.h, Camera.h, Render.cuh:357-557); error behaviour is stricter:
// failures throw crt::Error / return a crt_status instead of printing and
// continuing.
#ifndef CRT_HOST_HPP
#define CRT_HOST_HPP

#include "../../include/crt.h"

#include <cstdint>
#include <stdexcept>
#include <map>
#include <string>
#include <vector>

namespace crt {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};

struct Vec3 {
    float x = 0.0f, y = 0.0f, z = 0.0f;
};

enum Illum { DIFFUSE = 0, SPECULAR = 1 }; // reference: include/Material.h:7-10

// reference: include/Material.h:11-77 (ks / ka are never read downstream)
class Material {
public:
    Material();
    Material(Vec3 kd, Vec3 ke, float ns, Illum mode);
    Vec3 get_kd() const { return kd_; }
    Vec3 get_ke() const { return ke_; }
    float get_ns() const { return ns_; }
    bool has_emission() const { return has_emit_; }
    Illum get_mode() const { return mode_; }
    bool same_as(const Material& o) const;

private:
    Vec3 kd_, ke_;
    float ns_;
    bool has_emit_;
    Illum mode_;
};

// reference: include/Triangle.h:9-132
class Triangle {
public:
    Triangle(Vec3 v1, Vec3 v2, Vec3 v3, const Material& m);
    Vec3 get_v1() const { return v1_; }
    Vec3 get_v2() const { return v2_; }
    Vec3 get_v3() const { return v3_; }
    Vec3 get_normal() const { return normal_; }
    Vec3 get_center() const { return center_; }
    float get_area() const { return area_; }
    float get_area_of_obj() const { return area_of_obj_; }
    void set_area_of_obj(float a) { area_of_obj_ = a; }
    const Material& get_material() const { return material_; }
    Vec3 get_min() const { return lo_; }
    Vec3 get_max() const { return hi_; }
    // the object of the scene the triangle came with (Scene::add_*_obj numbers them; Scene::transform_object finds its triangles by it)
    uint32_t get_object() const { return object_; }
    void set_object(uint32_t o) { object_ = o; }

private:
    Vec3 v1_, v2_, v3_, center_, normal_, lo_, hi_;
    Material material_;
    float area_ = 0.0f, area_of_obj_ = 0.0f;
    uint32_t object_ = 0;
};

// reference: include/Object.h:7-31
class Object {
public:
    explicit Object(const std::vector<Triangle>& ts);
    std::vector<Triangle>& get_triangles() { return triangles_; }
    const std::vector<Triangle>& get_triangles() const { return triangles_; }
    float get_area() const { return area_; }

private:
    std::vector<Triangle> triangles_;
    float area_ = 0.0f;
};

// reference: include/BVH.h:9-20
struct BVHNode {
    int lc = -1, rc = -1;
    unsigned n = 0;
    int it = -1;
    Vec3 AA, BB;
};

// reference: include/BVH.h:22-120.  Reorders `triangles` in place, emits
// nodes in post-order (root last).
class BVH {
public:
    BVH(unsigned thresh_n, std::vector<Triangle>& triangles);
    // the same tree built on GPU `device` (csrc/crt_bvh_build.hip), byte-identical node and triangle arrays; ranges with equal
    // sort keys are finished by build_node on the host
    BVH(unsigned thresh_n, std::vector<Triangle>& triangles, int device, crt_bvh_build_info* info);
    int get_root_index() const { return root_; }
    size_t get_nodes_size() const { return nodes_.size(); }
    const std::vector<BVHNode>& get_nodes() const { return nodes_; }
    const std::vector<Triangle>& get_triangles() const { return triangles_; }
    size_t get_triangles_size() const { return triangles_.size(); }
    unsigned max_depth() const { return max_depth_; }
    // The boxes of the tree as it stands from the triangles as they now are (crt_scene_refit's rule, include/crt.h): a leaf's from the
    // nine coordinates of each of its triangles, an inner node's as the union of its children's, in the order in which -0 < +0
    void refit();

private:
    struct Key { float c[3]; uint32_t idx; };
    int build_node(std::vector<Key>& keys, int l, int r, unsigned depth);
    unsigned thresh_n_;
    int root_ = -1;
    unsigned max_depth_ = 0;
    std::vector<Triangle>& triangles_;
    std::vector<BVHNode> nodes_;
};

// reference: include/Scene.h:16-102
class Scene {
public:
    Scene(unsigned width, unsigned height);
    ~Scene();
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    void add_light_obj(Object& obj);
    void add_normal_obj(Object& obj);
    void set_BVH(unsigned thresh_n);
    void set_BVH_device(unsigned thresh_n, int device, crt_bvh_build_info* info = nullptr);
    // A 3 x 4 affine map (row-major: x' = m[0] x + m[1] y + m[2] z + m[3], ...) on the vertices of object `index` (get_objects' order),
    // in the scene's triangles and in the light's own copies.  A term whose coefficient is 0 is left out, so the identity keeps every
    // bit, -0 included.  normal, area and area_of_obj are recomputed as the loader computes them (Triangle, Object); the BVH keeps its
    // topology and triangle order, and its boxes are refitted (BVH::refit).  set_BVH afterwards builds a new tree as ever.
    void transform_object(unsigned index, const float m[12]);
    void free();
    unsigned get_height() const { return height_; }
    unsigned get_width() const { return width_; }
    unsigned get_pixels() const { return width_ * height_; }
    void set_height(unsigned h) { height_ = h; }
    void set_width(unsigned w) { width_ = w; }
    BVH& get_bvh();
    bool has_bvh() const { return bvh_ != nullptr; }
    std::vector<Object>& get_light_objs() { return light_objs_; }
    std::vector<Triangle>& get_triangles() { return triangles_; }
    // every object in creation order (normal and light interleaved) with a light flag
    const std::vector<std::pair<bool, Object>>& get_objects() const { return objects_; }

    // Flat, upload-ready view (valid until the scene changes); builds the
    // de-duplicated material table on first use after set_BVH.
    const crt_scene_desc& flat();

private:
    unsigned width_, height_;
    BVH* bvh_ = nullptr;
    std::vector<Object> light_objs_;
    std::vector<std::pair<bool, Object>> objects_;
    std::vector<Triangle> triangles_;
    // flat storage
    bool flat_valid_ = false;
    std::vector<crt_bvh_node> f_nodes_;
    std::vector<crt_triangle> f_tris_, f_light_tris_;
    std::vector<crt_material> f_mats_;
    std::vector<crt_light> f_lights_;
    crt_scene_desc desc_{};
};

// reference: include/Loader.h:13-131 + include/OBJLoader.h:12-229
class Loader {
public:
    void read_OBJ(const char* obj_path, const char* mtl_dir);
    void load_object(uint64_t index, std::vector<Triangle>& triangles, std::vector<Triangle>& light_triangles) const;
    uint64_t size() const { return shapes_.size(); }

private:
    struct Shape {
        std::string material_id;
        std::vector<uint64_t> faces; // 3 vertex indices per face (only the first three of an `f` line are kept)
        float kd[3] = {0, 0, 0}, ke[3] = {0, 0, 0};
        float ns = 1.0f;
        bool has_map_kd = false;
        std::string map_kd;          // mtl_dir + "/" + file name (OBJLoader.h:184-193)
    };
    struct Texture {                 // what stbi_load returns (Loader.h:58): x, y, components, 8-bit samples
        int x = 0, y = 0, comp = 0;
        std::vector<uint8_t> px;
    };
    const Texture& texture(const std::string& path) const;
    std::vector<Shape> shapes_;
    std::vector<Vec3> vertices_;
    std::vector<float> textures_;    // u, v per `vt` line (OBJLoader.h:88-93)
    size_t n_normals_ = 0;
    mutable std::map<std::string, Texture> tex_cache_;
};

// reference: include/Camera.h:9-36; out is column-major
void get_inverse_view_matrix(const float eye[3], const float lookat[3], const float up[3], float out[9]);

// reference: src/main.cu:40-90.  all_objs (optional): every (OBJ_path, MTL_dir) pair of the file -- the crt_task POD holds the first eight
typedef std::vector<std::pair<std::string, std::string>> TaskObjs;
crt_task load_task(const std::string& config_path, TaskObjs* all_objs = nullptr);
// loads every OBJ of a task into `scene` the way render_view does (src/main.cu:122-145); all_objs as returned by load_task when the
// file names more than eight
void load_task_scene(const crt_task& task, Scene& scene, const std::string& base_dir, const TaskObjs* all_objs = nullptr);

// reference: include/Render.cuh:357-557.  Drives the device layer through the C ABI.
class Render {
public:
    Render(Scene* scene, unsigned spp = 16, float P_RR = 0.8f, unsigned light_sample_n = 1, int device = 0);
    // one rank per entry of `devices` (crt_multi: tile shards, one RCCL all-gather); gather = CRT_GATHER_*
    Render(Scene* scene, unsigned spp, float P_RR, unsigned light_sample_n, const std::vector<int>& devices, uint32_t gather = CRT_GATHER_AUTO);
    ~Render();
    Render(const Render&) = delete;
    Render& operator=(const Render&) = delete;
    // run_view(eye_pos, inv_view_mat, fovY): inv_view column-major, fovY in radians
    void run_view(const float eye_pos[3], const float inv_view_mat[9], float fovY);
    // run_view on a multi-device Render with more of the frame's buffers, gathered from all ranks on the way (crt_multi_render_buffers):
    // want names the planes (CRT_MULTI_* bits; RGB and MEAN are always made).  Frame and mean buffers as run_view leaves them, albedo,
    // normal, depth, emission and diffuse_albedo in the buffers of run_aov; get_gathered_buffer(CRT_MULTI_x) is plane x of the last call --
    // W x H pixels of its type, row 0 = image top -- or nullptr if that call did not make it (or run_view has run since).  The
    // single-device methods keep refusing a multi-device Render; a single-device Render refuses this one (CRT_ERR_UNSUPPORTED).
    void run_view_gathered(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t want);
    const void* get_gathered_buffer(uint32_t plane) const;
    // the adaptive frame of crt_render_adaptive (ap: crt_adaptive_defaults with overrides) in place of run_view's: frame and mean buffers as
    // run_view leaves them, the samples per pixel in get_samples_buffer, and with want_variance the variance of the mean in variance();
    // CRT_FLAG_STATS / _BOUNDED_RADIANCE do not apply; one device only
    void run_view_adaptive(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_adaptive_params& ap, bool want_variance = false);
    // the frame of crt_render_map (sample_map: W x H counts, row 0 = image top; sample_begin > 0 continues the frame in flight) and of
    // crt_render_planned (ap.step_samples is ignored): buffers as run_view_adaptive leaves them, the call's figures in last_map_info
    void run_view_map(const float eye_pos[3], const float inv_view_mat[9], float fovY, const uint32_t* sample_map, uint32_t sample_begin = 0, bool want_variance = false);
    void run_view_planned(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_adaptive_params& ap, bool want_variance = false);
    const crt_map_info& last_map_info() const { return map_info_; }
    // the host scene's current triangles into the device handle without rebuilding it (crt_scene_refit): after Scene::transform_object.
    // Ends the frame in flight; one device only
    crt_refit_info refit();
    // the error of the frame in flight, or of the last finished frame, against the adaptive call's target (crt_frame_error): reads only
    crt_frame_error_info frame_error(float threshold, float mean_floor);
    // a uniform frame rendered until it is clean enough (crt_render_until; up: crt_until_defaults with overrides): frame and mean buffers
    // as run_view leaves them when the frame ran to spp, else the preview's at last_until_info().samples_done, and then the frame stays
    // in flight: run_view_until with sample_begin = samples_done continues it.  want_variance: the variance of that mean in variance()
    void run_view_until(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_until_params& up, uint32_t sample_begin = 0, bool want_variance = false);
    const crt_until_info& last_until_info() const { return until_info_; }
    const uint32_t* get_samples_buffer() const { return samples_buffer_.data(); } // W x H, after run_view_adaptive / _map / _planned
    const crt_adaptive_info& last_adaptive_info() const { return adaptive_info_; }
    // first-hit albedo, normal and depth of the frame run_view draws with the same camera and settings (crt_render_aov); one device only
    void run_aov(const float eye_pos[3], const float inv_view_mat[9], float fovY);
    const float* get_albedo_buffer() const { return albedo_buffer_.data(); } // W x H x 3, row 0 = image top
    const float* get_normal_buffer() const { return normal_buffer_.data(); } // W x H x 3
    const float* get_depth_buffer() const { return depth_buffer_.data(); }   // W x H
    const crt_aov_info& last_aov_info() const { return aov_info_; }
    // on: run_aov also fills the shading AOVs from its one trace (crt_render_aov_shading): emission and diffuse_albedo, W x H x 3 each
    void set_aov_shading(bool on) { aov_shading_ = on; }
    const float* get_emission_buffer() const { return emission_buffer_.data(); }
    const float* get_diffuse_albedo_buffer() const { return diffuse_albedo_buffer_.data(); }
    // the direct-light AOVs of the frame run_view draws with the same camera and settings (crt_render_aov_direct): the first-vertex
    // next-event term of the frame's own paths, its unshadowed form, its variance and the visible fraction of its samples; one device only
    void run_view_aov_direct(const float eye_pos[3], const float inv_view_mat[9], float fovY);
    const float* get_direct_buffer() const { return direct_buffer_.data(); }                   // W x H x 3, row 0 = image top
    const float* get_unshadowed_buffer() const { return unshadowed_buffer_.data(); }           // W x H x 3
    const float* get_direct_variance_buffer() const { return direct_variance_buffer_.data(); } // W x H x 3
    const float* get_visibility_buffer() const { return visibility_buffer_.data(); }           // W x H
    const crt_aov_info& last_aov_direct_info() const { return aov_direct_info_; }
    // the ambient-occlusion AOVs of the frame run_view draws with the same camera and settings (crt_render_aov_ao): ao_samples rays of
    // at most max_distance over the hemisphere of every first hit; 0 takes crt_aov_ao_defaults' value for either; one device only
    void run_view_aov_ao(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t ao_samples = 0, float max_distance = 0.0f);
    const float* get_ao_buffer() const { return ao_buffer_.data(); }                   // W x H, row 0 = image top
    const float* get_openness_buffer() const { return openness_buffer_.data(); }       // W x H
    const float* get_bent_normal_buffer() const { return bent_normal_buffer_.data(); } // W x H x 3
    const crt_aov_info& last_aov_ao_info() const { return aov_ao_info_; }
    // on: the filters and the temporal pass work on irradiance (crt_demodulate / crt_modulate with albedo_floor and the shading AOVs of
    // the last run_aov, which set_demodulate therefore switches on).  run_denoise / run_denoise_var demodulate the frame (and its
    // variance), filter, and modulate the result.  run_temporal / run_temporal_moments demodulate each frame before the blend, so the
    // history, get_temporal_mean_buffer() and get_temporal_variance_buffer() hold irradiance, while get_temporal_buffer() (RGB8) is the
    // accumulated frame modulated with the current frame's buffers; run_denoise_temporal filters the irradiance and modulates.  A
    // change of the switch starts a history.
    void set_demodulate(bool on, float albedo_floor = 0.0f) { demodulate_ = on; albedo_floor_ = albedo_floor; if (on) aov_shading_ = true; }
    // the AOVs that follow mirror bounces (crt_render_aov_specular; max_bounces 0: crt_aov_specular_defaults'); one device only.
    // as_albedo_guide: guide_albedo also replaces the albedo of the last run_aov as the guide of run_denoise / run_denoise_var
    void run_aov_specular(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t max_bounces = 0, bool as_albedo_guide = false);
    const float* get_guide_albedo_buffer() const { return guide_albedo_buffer_.data(); } // W x H x 3
    const float* get_last_normal_buffer() const { return last_normal_buffer_.data(); }   // W x H x 3
    const float* get_path_depth_buffer() const { return path_depth_buffer_.data(); }     // W x H
    const float* get_bounces_buffer() const { return bounces_buffer_.data(); }           // W x H
    const crt_aov_info& last_aov_specular_info() const { return aov_specular_info_; }
    // the frame of the last run_view filtered by crt_denoise with the albedo, normal and depth of the last run_aov as guides (call both
    // first, with the same camera); prm: crt_denoise_defaults with overrides, its width and height are set here; one device only
    void run_denoise(const crt_denoise_params& prm);
    // the same with the variance-guided filter (crt_denoise_var; prm: crt_denoise_var_defaults with overrides): the last run_view must
    // have had CRT_FLAG_VARIANCE (set_flags)
    void run_denoise_var(const crt_denoise_params& prm);
    // the same with the non-local-means filter (crt_denoise_nlm; prm: crt_denoise_nlm_defaults with overrides), CRT_FLAG_VARIANCE likewise
    void run_denoise_nlm(const crt_nlm_params& prm);
    // the same with the feature-regression filter (crt_denoise_regress; prm: crt_denoise_regress_defaults with overrides), CRT_FLAG_VARIANCE
    // likewise; with set_demodulate the albedo feature is taken off the mask.  last_regress_info(): its timer and fallback pixels
    void run_denoise_regress(const crt_regress_params& prm);
    const crt_regress_info& last_regress_info() const { return regress_info_; }
    // Multi-scale denoising: run_denoise_var, run_denoise_nlm and run_denoise_regress run their filter at n scales of a Laplacian pyramid
    // (crt_pyramid_down of the frame, its variance and the guides n - 1 times, the filter with the same settings at every scale,
    // crt_pyramid_merge from the coarsest scale up), where the single call stands: it composes with set_demodulate.  n is 1 .. 4; 1 (the
    // default) is the single call.  last_denoise_info() then holds the sum of the calls' timers, last_regress_info() the finest scale's.
    void set_denoise_scales(unsigned n);
    // Error-estimated filter selection (crt_half_buffers, crt_filter_select): the last run_view must have had CRT_FLAG_HALF_BUFFERS
    // (set_flags).  candidates: 1 .. 4 of SELECT_NONE / _ATROUS / _VAR / _NLM / _REG, each run with its own defaults on either half frame,
    // the variance-taking ones with 2 x variance(), _REG with its weights from the other half frame; prm: crt_filter_select_defaults with
    // overrides, its sizes and n_candidates are set here.
    // The result is the denoised buffer; the choice map is get_choice_buffer().  Not with set_demodulate.
    enum { SELECT_NONE = 0, SELECT_ATROUS = 1, SELECT_VAR = 2, SELECT_NLM = 3, SELECT_REG = 4 };
    void run_denoise_select(const std::vector<int>& candidates, const crt_filter_select_params& prm);
    const crt_filter_select_info& last_select_info() const { return select_info_; }
    const std::vector<unsigned char>& get_choice_buffer() const { return choice_buffer_; }
    // per-pixel variance of the mean of the last run_view (crt_variance; needs set_flags(CRT_FLAG_VARIANCE) before it): W x H x 3,
    // fetched from the device on the first call after a frame; one device only
    const float* variance();
    // Pixel reconstruction filters (crt_set_pixel_filter, crt_filtered_frame): the filter of this Render's handle -- nullptr: none -- and,
    // after a run_view with set_flags(CRT_FLAG_PIXEL_FILTER), the frame under it: get_filtered_buffer (W x H x 3 RGB8) and
    // get_filtered_mean_buffer (W x H x 3).  One device only.
    void set_pixel_filter(const crt_pixel_filter* filter);
    void filtered_frame();
    const unsigned char* get_filtered_buffer() const { return filtered_buffer_.data(); }
    const float* get_filtered_mean_buffer() const { return filtered_mean_buffer_.data(); }
    void save_filtered_buffer(const char* save_path) const;
    // One frame of a temporally accumulated sequence (crt_temporal; prm: crt_temporal_defaults with overrides, its sizes and cameras are set
    // here): run_view (needs set_flags(CRT_FLAG_VARIANCE)), variance, run_aov, then the frame is blended into the history this object keeps
    // -- colour, variance, history length, depth, normal, material ID and camera of the previous call -- and the unfiltered result becomes
    // the new history.  The first call, the first after reset_temporal() or after a change of size starts a history.  Render every frame
    // with another seed (set_seed).  frame and mean buffers hold the frame as rendered; one device only.  clamp != nullptr: the history is
    // clamped to its neighbourhood (crt_temporal_clamped); last_temporal_clamped() is then the count of pixels it moved
    void run_temporal(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm, const crt_temporal_clamp* clamp = nullptr);
    // run_temporal with a second reprojection for what mirrors show (crt_temporal_dual; dual: crt_temporal_dual_defaults with overrides): each
    // frame also runs run_aov_specular(max_bounces; 0: its default) -- not as the albedo guide --, its path_depth, bounces and last_normal
    // are kept with the history, and last_temporal_dual_info() has the four counts (last_temporal_info() and last_temporal_clamped() are
    // filled from it).  A history made by run_temporal is not continued, nor the other way round.
    void run_temporal_specular(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm, const crt_temporal_clamp* clamp,
                               const crt_temporal_dual_params& dual, uint32_t max_bounces = 0);
    const crt_temporal_dual_info& last_temporal_dual_info() const { return temporal_dual_info_; }
    // run_temporal with the variance measured instead of carried: the frame needs no CRT_FLAG_VARIANCE (one sample per pixel works), the
    // history also keeps the moment planes of crt_temporal_moments, and get_temporal_variance_buffer() -- what run_denoise_temporal
    // filters with -- is crt_variance_estimate of them with the frame's normal and depth (est: crt_variance_estimate_defaults with
    // overrides, its sizes are set here).  A history made by run_temporal is not continued, nor the other way round.
    void run_temporal_moments(const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm, const crt_temporal_clamp* clamp,
                              const crt_variance_estimate_params& est);
    const crt_variance_estimate_info& last_variance_estimate_info() const { return estimate_info_; }
    void reset_temporal() { temporal_valid_ = false; }
    const unsigned char* get_temporal_buffer() const { return temporal_rgb_.data(); }        // W x H x 3 RGB8: the accumulated frame
    const float* get_temporal_mean_buffer() const { return temporal_color_.data(); }          // W x H x 3
    const float* get_temporal_variance_buffer() const { return temporal_variance_.data(); }   // W x H x 3
    const float* get_temporal_history_buffer() const { return temporal_history_.data(); }     // W x H: frames accumulated per pixel
    const crt_temporal_info& last_temporal_info() const { return temporal_info_; }
    uint64_t last_temporal_clamped() const { return temporal_clamped_; }
    // the accumulated frame filtered by crt_denoise_var with its accumulated variance and the guides of the last frame
    void run_denoise_temporal(const crt_denoise_params& prm);
    void save_temporal_buffer(const char* save_path) const;
    // Resolution scaling (crt_upsample; prm: crt_upsample_defaults with overrides, its sizes are set here): the frame's paths at
    // (W / factor, H / factor) with its variance, the shading AOVs with albedo, normal and depth at that size and at (W, H) -- there with
    // guide_spp samples per pixel, 0: the frame's --, the low frame demodulated with the low buffers, upsampled along the two sets of
    // guides and modulated with the full-resolution buffers.  factor is 2 .. 8 and divides both sides.  The AOV buffers are then those
    // of a run_aov with set_aov_shading at (W, H); frame and mean buffers are untouched; the handle's sums are the low frame's.  One
    // device only.
    void run_view_upsampled(const float eye_pos[3], const float inv_view_mat[9], float fovY, unsigned factor, const crt_upsample_params& prm, unsigned guide_spp = 0);
    const unsigned char* get_upsampled_buffer() const { return upsampled_buffer_.data(); }   // W x H x 3 RGB8
    const float* get_upsampled_mean_buffer() const { return upsampled_mean_buffer_.data(); } // W x H x 3
    const crt_upsample_info& last_upsample_info() const { return upsample_info_; }
    void save_upsampled_buffer(const char* save_path) const;
    const unsigned char* get_denoised_buffer() const { return denoised_buffer_.data(); } // W x H x 3 RGB8
    const float* get_denoised_mean_buffer() const { return denoised_mean_buffer_.data(); } // W x H x 3
    const crt_denoise_info& last_denoise_info() const { return denoise_info_; }
    void save_denoised_buffer(const char* save_path) const;
    void free();
    void save_frame_buffer(const char* save_path) const;
    unsigned char* get_frame_buffer() const { return const_cast<unsigned char*>(frame_buffer_.data()); }
    const float* get_mean_buffer() const { return mean_buffer_.data(); }
    void set_spp(const int& spp) { spp_ = (unsigned)spp; }
    void set_P_RR(const float& p) { P_RR_ = p; }
    void set_light_sample_n(const int& n) { light_sample_n_ = (unsigned)n; }
    void set_seed(uint64_t s) { seed_ = s; }
    void set_traversal(uint32_t t) { traversal_ = t; }
    void set_flags(uint32_t f) { flags_ = f; } // CRT_FLAG_* of crt_params that a caller may choose: CRT_FLAG_TRACE_ALL, CRT_FLAG_BOUNDED_RADIANCE, CRT_FLAG_VARIANCE, CRT_FLAG_HALF_BUFFERS, CRT_FLAG_PIXEL_FILTER
    void set_width(const unsigned& w);
    void set_height(const unsigned& h);
    const crt_stats& last_stats() const { return stats_; }
    // multi-device renders: what the exchange ran on (n_ranks == 0 for a single-device Render) and the ranks' own statistics
    const crt_multi_info& last_multi_info() const { return multi_info_; }
    const std::vector<crt_stats>& last_rank_stats() const { return rank_stats_; }

private:
    Scene* scene_;
    unsigned spp_, light_sample_n_;
    float P_RR_;
    uint64_t seed_ = 0;
    uint32_t traversal_ = CRT_TRAVERSAL_EXACT;
    uint32_t flags_ = 0;
    crt_scene* device_scene_ = nullptr;
    crt_multi* multi_ = nullptr;
    crt_multi_info multi_info_{};
    std::vector<crt_stats> rank_stats_;
    std::vector<unsigned char> frame_buffer_;
    std::vector<float> mean_buffer_;
    std::vector<float> albedo_buffer_, normal_buffer_, depth_buffer_;
    std::vector<unsigned char> denoised_buffer_;
    std::vector<float> denoised_mean_buffer_;
    std::vector<float> variance_buffer_; // empty until variance() has fetched it for the last frame (run_view_adaptive fills it itself)
    std::vector<uint32_t> samples_buffer_;
    std::vector<unsigned char> filtered_buffer_; // filtered_frame
    std::vector<float> filtered_mean_buffer_;
    std::vector<int32_t> material_buffer_; // run_aov
    uint32_t gathered_ = 0;                // run_view_gathered: the planes the last call made
    std::vector<float> half_a_buffer_, half_b_buffer_, coverage_buffer_;
    std::vector<int32_t> tri_buffer_;
    void sum_rank_stats();
    // run_temporal: the accumulated frame = the next call's history, with the guides and the camera it was made with
    std::vector<float> temporal_color_, temporal_variance_, temporal_history_, temporal_depth_, temporal_normal_;
    std::vector<int32_t> temporal_id_;
    std::vector<unsigned char> temporal_rgb_;
    crt_camera temporal_cam_{};
    unsigned temporal_width_ = 0, temporal_height_ = 0;
    bool temporal_valid_ = false;
    crt_temporal_info temporal_info_{};
    uint64_t temporal_clamped_ = 0;
    std::vector<float> temporal_m1_, temporal_m2_;   // run_temporal_moments: the history's moment planes
    bool temporal_moments_ = false;                  // the history was made by run_temporal_moments
    std::vector<float> temporal_path_depth_, temporal_bounces_, temporal_last_normal_;   // run_temporal_specular: the history's specular planes
    bool temporal_specular_ = false;                 // the history was made by run_temporal_specular
    crt_temporal_dual_info temporal_dual_info_{};
    crt_variance_estimate_info estimate_info_{};
    unsigned denoise_scales_ = 1;                    // set_denoise_scales
    // a single-frame filter with its settings: kind is SELECT_ATROUS .. SELECT_REG, and the settings of that kind are the ones that count
    struct Filter {
        int kind;
        crt_denoise_params dn{};                     // SELECT_ATROUS, SELECT_VAR
        crt_nlm_params nlm{};
        crt_regress_params reg{};
    };
    static Filter default_filter(int kind);          // every kind's settings as the library's defaults fill them
    int apply_filter(const Filter& f, uint32_t w, uint32_t h, const crt_pyramid_planes& in, const float* weights, float* out_mean, unsigned char* out_rgb,
                     crt_denoise_info* info);
    void filter_scales(const char* who, const Filter& f, unsigned scales, uint32_t w, uint32_t h, const crt_pyramid_planes& in, float* out_mean, unsigned char* out_rgb);
    void denoise_of(const char* who, Filter f, const float* color, const float* variance, bool is_irradiance, unsigned scales);
    // set_aov_shading / set_demodulate
    bool aov_shading_ = false, demodulate_ = false;
    float albedo_floor_ = 0.0f;
    bool temporal_demodulated_ = false;              // the history holds irradiance
    std::vector<float> emission_buffer_, diffuse_albedo_buffer_;
    crt_modulate_params modulate_params(const char* who) const;
    void demodulate_of(const char* who, const float* color, const float* variance, std::vector<float>& irradiance, std::vector<float>& irradiance_variance) const;
    void modulate_of(const char* who, const float* irradiance, float* out_mean, unsigned char* out_rgb) const;
    crt_adaptive_info adaptive_info_{};
    crt_map_info map_info_{};
    crt_until_info until_info_{};
    void view_args(const float eye_pos[3], const float inv_view_mat[9], float fovY, uint32_t flags, crt_camera& cam, crt_params& p) const;
    template <class Call> void sampled_frame(const char* who, const float eye_pos[3], const float inv_view_mat[9], float fovY, bool want_variance, Call render);
    int device_ = 0;
    crt_denoise_info denoise_info_{};
    crt_regress_info regress_info_{};
    crt_filter_select_info select_info_{};
    std::vector<unsigned char> choice_buffer_;
    crt_stats stats_{};
    crt_aov_info aov_info_{};
    std::vector<float> guide_albedo_buffer_, last_normal_buffer_, path_depth_buffer_, bounces_buffer_; // run_aov_specular
    crt_aov_info aov_specular_info_{};
    std::vector<float> direct_buffer_, unshadowed_buffer_, direct_variance_buffer_, visibility_buffer_; // run_view_aov_direct
    crt_aov_info aov_direct_info_{};
    std::vector<float> ao_buffer_, openness_buffer_, bent_normal_buffer_; // run_view_aov_ao
    crt_aov_info aov_ao_info_{};
    std::vector<unsigned char> upsampled_buffer_;    // run_view_upsampled
    std::vector<float> upsampled_mean_buffer_;
    crt_upsample_info upsample_info_{};
    // the rules the methods share, each stated once (crt_host_render.cpp); hidden: no symbols of the library
    __attribute__((visibility("hidden"))) void alive(const char* who) const;
    __attribute__((visibility("hidden"))) void one_device(const char* who, const char* noun) const;
    __attribute__((visibility("hidden"))) void need_guides(const std::string& who) const;
    template <class Blend> void temporal_frame(const char* who, const float eye_pos[3], const float inv_view_mat[9], float fovY, const crt_temporal_params& prm, bool moments,
                                               const float* var, Blend blend, bool specular);
};

} // namespace crt
#endif
