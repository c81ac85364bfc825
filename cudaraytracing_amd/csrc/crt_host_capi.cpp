// cudaraytracing_amd/csrc/crt_host_capi.cpp -- the host half of the C ABI (include/crt.h) over the classes of crt_host.hpp: host scenes,
// tasks, images, the status texts and the last error; the PNG and PFM writers.
#include "crt_host.hpp"
#include "crt_image.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

// =========================================================== C ABI (host) ==
namespace {
thread_local std::string g_last_error;
}
extern "C" void crt_set_last_error_(const char* msg) { g_last_error = msg ? msg : ""; }

struct crt_host_scene {
    crt::Scene scene;
    crt_host_scene(uint32_t w, uint32_t h) : scene(w, h) {}
};

#define CRT_HOST_TRY(...)                                                                   \
    try { __VA_ARGS__; return CRT_OK; }                                                            \
    catch (const crt::Error& e) { g_last_error = e.what(); return e.status; }               \
    catch (const std::bad_alloc&) { g_last_error = "out of host memory"; return CRT_ERR_OOM; } \
    catch (const std::exception& e) { g_last_error = e.what(); return CRT_ERR_INVALID_ARG; }

extern "C" {

const char* crt_strerror(int status)
{
    switch (status) {
    case CRT_OK: return "ok";
    case CRT_ERR_INVALID_ARG: return "invalid argument";
    case CRT_ERR_NO_DEVICE: return "no HIP device";
    case CRT_ERR_HIP: return "HIP runtime error";
    case CRT_ERR_UNSUPPORTED: return "unsupported";
    case CRT_ERR_IO: return "I/O error";
    case CRT_ERR_PARSE: return "parse error";
    case CRT_ERR_OOM: return "out of memory";
    default: return "unknown status";
    }
}
const char* crt_last_error(void) { return g_last_error.c_str(); }
int crt_abi_version(void) { return CRT_ABI_VERSION; }

int crt_host_scene_create(uint32_t width, uint32_t height, crt_host_scene** out)
{
    if (!out || width == 0 || height == 0) { g_last_error = "crt_host_scene_create: bad arguments"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY(*out = new crt_host_scene(width, height));
}
int crt_host_scene_destroy(crt_host_scene* s)
{
    delete s;
    return CRT_OK;
}
int crt_host_scene_add_obj(crt_host_scene* s, const char* obj_path, const char* mtl_dir)
{
    if (!s || !obj_path || !mtl_dir) { g_last_error = "crt_host_scene_add_obj: null argument"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY({
        crt::Loader loader;
        loader.read_OBJ(obj_path, mtl_dir);
        std::vector<crt::Triangle> tris, light_tris;
        for (uint64_t i = 0; i < loader.size(); i++) {
            loader.load_object(i, tris, light_tris);
            if (!tris.empty()) { crt::Object o(tris); s->scene.add_normal_obj(o); }
            if (!light_tris.empty()) { crt::Object o(light_tris); s->scene.add_light_obj(o); }
        }
    });
}
int crt_host_scene_set_bvh(crt_host_scene* s, uint32_t thresh_n)
{
    if (!s) { g_last_error = "crt_host_scene_set_bvh: null scene"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY(s->scene.set_BVH(thresh_n));
}
int crt_host_scene_set_bvh_device(crt_host_scene* s, uint32_t thresh_n, int device, crt_bvh_build_info* info)
{
    if (!s) { g_last_error = "crt_host_scene_set_bvh_device: null scene"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY(s->scene.set_BVH_device(thresh_n, device, info));
}
int crt_host_scene_desc(const crt_host_scene* s, crt_scene_desc* out)
{
    if (!s || !out) { g_last_error = "crt_host_scene_desc: null argument"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY(*out = const_cast<crt_host_scene*>(s)->scene.flat());
}
int crt_host_scene_transform_object(crt_host_scene* s, uint32_t index, const float m[12])
{
    if (!s || !m) { g_last_error = "crt_host_scene_transform_object: null argument"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY(s->scene.transform_object(index, m));
}
int crt_host_scene_num_objects(const crt_host_scene* s, uint32_t* n)
{
    if (!s || !n) { g_last_error = "crt_host_scene_num_objects: null argument"; return CRT_ERR_INVALID_ARG; }
    *n = (uint32_t)s->scene.get_objects().size();
    return CRT_OK;
}
int crt_host_scene_object(const crt_host_scene* s, uint32_t index, float* area, int32_t* is_light, uint32_t* n_tris)
{
    if (!s || index >= s->scene.get_objects().size()) { g_last_error = "crt_host_scene_object: bad index"; return CRT_ERR_INVALID_ARG; }
    const auto& o = s->scene.get_objects()[index];
    if (area) *area = o.second.get_area();
    if (is_light) *is_light = o.first ? 1 : 0;
    if (n_tris) *n_tris = (uint32_t)o.second.get_triangles().size();
    return CRT_OK;
}
int crt_inverse_view(const float eye[3], const float lookat[3], const float up[3], float out[9])
{
    if (!eye || !lookat || !up || !out) { g_last_error = "crt_inverse_view: null argument"; return CRT_ERR_INVALID_ARG; }
    crt::get_inverse_view_matrix(eye, lookat, up, out);
    return CRT_OK;
}
int crt_image_load(const char* path, int32_t* x, int32_t* y, int32_t* comp, uint8_t* out, uint64_t cap)
{
    if (!path || !x || !y || !comp) { g_last_error = "crt_image_load: null argument"; return CRT_ERR_INVALID_ARG; }
    try {
        crtimg::Image img;
        const std::string err = crtimg::load(path, img);
        if (!err.empty()) { g_last_error = "crt_image_load: " + err; return err.rfind("cannot open", 0) == 0 ? CRT_ERR_IO : CRT_ERR_UNSUPPORTED; }
        *x = img.width; *y = img.height; *comp = img.comp;
        if (out) {
            if (cap < img.px.size()) { g_last_error = "crt_image_load: buffer too small"; return CRT_ERR_INVALID_ARG; }
            std::memcpy(out, img.px.data(), img.px.size());
        }
        return CRT_OK;
    } catch (const std::bad_alloc&) { // (a file may honestly announce more pixels than the host has memory for)
        g_last_error = "crt_image_load: out of host memory";
        return CRT_ERR_OOM;
    }
}
int crt_task_load(const char* path, crt_task* out)
{
    if (!path || !out) { g_last_error = "crt_task_load: null argument"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY(*out = crt::load_task(path));
}
int crt_task_obj(const char* path, uint32_t index, char* obj_path, char* mtl_dir, uint32_t cap)
{
    if (!path || !obj_path || !mtl_dir) { g_last_error = "crt_task_obj: null argument"; return CRT_ERR_INVALID_ARG; }
    CRT_HOST_TRY({
        crt::TaskObjs all;
        (void)crt::load_task(path, &all);
        if (index >= all.size()) throw crt::Error(CRT_ERR_INVALID_ARG, "crt_task_obj: index beyond the file's OBJ_paths");
        if (all[index].first.size() + 1 > cap || all[index].second.size() + 1 > cap) throw crt::Error(CRT_ERR_INVALID_ARG, "crt_task_obj: buffer too small");
        std::memcpy(obj_path, all[index].first.c_str(), all[index].first.size() + 1);
        std::memcpy(mtl_dir, all[index].second.c_str(), all[index].second.size() + 1);
    });
}

// ---- PNG (stored deflate blocks; replaces stbi_write_png, Render.cuh:489-493) ----
static uint32_t crc_table[256];
static bool crc_ready = false;
static uint32_t crc32_update(uint32_t c, const uint8_t* p, size_t n)
{
    if (!crc_ready) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t k = i;
            for (int j = 0; j < 8; j++) k = (k & 1) ? 0xEDB88320u ^ (k >> 1) : k >> 1;
            crc_table[i] = k;
        }
        crc_ready = true;
    }
    for (size_t i = 0; i < n; i++) c = crc_table[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c;
}
static void put32(std::vector<uint8_t>& v, uint32_t x)
{
    v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x);
}
static void chunk(std::vector<uint8_t>& png, const char* type, const std::vector<uint8_t>& data)
{
    put32(png, (uint32_t)data.size());
    size_t start = png.size();
    png.insert(png.end(), type, type + 4);
    png.insert(png.end(), data.begin(), data.end());
    uint32_t c = crc32_update(0xffffffffu, png.data() + start, png.size() - start) ^ 0xffffffffu;
    put32(png, c);
}
int crt_write_png(const char* path, uint32_t width, uint32_t height, const uint8_t* rgb)
{
    if (!path || !rgb || width == 0 || height == 0) { g_last_error = "crt_write_png: bad arguments"; return CRT_ERR_INVALID_ARG; }
    std::vector<uint8_t> raw;
    raw.reserve((size_t)height * (3 * width + 1));
    for (uint32_t y = 0; y < height; y++) {
        raw.push_back(0); // filter: none
        raw.insert(raw.end(), rgb + (size_t)y * width * 3, rgb + (size_t)(y + 1) * width * 3);
    }
    std::vector<uint8_t> z;
    z.push_back(0x78); z.push_back(0x01);
    uint32_t a = 1, b = 0;
    size_t pos = 0;
    while (pos < raw.size() || raw.empty()) {
        size_t n = std::min<size_t>(65535, raw.size() - pos);
        z.push_back(pos + n >= raw.size() ? 1 : 0);
        z.push_back((uint8_t)(n & 0xff)); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 0xff)); z.push_back((uint8_t)((~n >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
        for (size_t i = 0; i < n; i++) { a = (a + raw[pos + i]) % 65521u; b = (b + a) % 65521u; }
        pos += n;
        if (raw.empty()) break;
    }
    put32(z, (b << 16) | a);
    std::vector<uint8_t> png = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<uint8_t> ihdr;
    put32(ihdr, width); put32(ihdr, height);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
    chunk(png, "IHDR", ihdr);
    chunk(png, "IDAT", z);
    chunk(png, "IEND", std::vector<uint8_t>());
    FILE* f = std::fopen(path, "wb");
    if (!f) { g_last_error = std::string("cannot open for writing: ") + path; return CRT_ERR_IO; }
    size_t w = std::fwrite(png.data(), 1, png.size(), f);
    std::fclose(f);
    if (w != png.size()) { g_last_error = std::string("short write: ") + path; return CRT_ERR_IO; }
    return CRT_OK;
}

int crt_write_pfm(const char* path, uint32_t width, uint32_t height, uint32_t channels, const float* data)
{
    if (!path || !data || width == 0 || height == 0 || (channels != 1 && channels != 3)) { g_last_error = "crt_write_pfm: bad arguments"; return CRT_ERR_INVALID_ARG; }
    static_assert(sizeof(float) == 4, "PFM samples are 32-bit floats");
    const uint32_t probe = 1;
    if (*(const uint8_t*)&probe != 1) { g_last_error = "crt_write_pfm: big-endian host"; return CRT_ERR_UNSUPPORTED; } // (scale -1.0 says little-endian)
    const std::string header = std::string(channels == 3 ? "PF" : "Pf") + "\n" + std::to_string(width) + " " + std::to_string(height) + "\n-1.0\n";
    FILE* f = std::fopen(path, "wb");
    if (!f) { g_last_error = std::string("cannot open for writing: ") + path; return CRT_ERR_IO; }
    bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size();
    const size_t row = (size_t)width * channels;
    for (uint32_t y = height; ok && y-- > 0;) // bottom row first
        ok = std::fwrite(data + (size_t)y * row, sizeof(float), row, f) == row;
    ok = std::fclose(f) == 0 && ok;
    if (!ok) { g_last_error = std::string("short write: ") + path; return CRT_ERR_IO; }
    return CRT_OK;
}

} // extern "C"
