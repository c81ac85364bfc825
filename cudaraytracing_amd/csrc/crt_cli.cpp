// crt_cli -- headless replacement of the reference's GUI shell for the hot path:
// reads a config.json (src/main.cu:67-90), ingests the OBJ/MTL files and builds the BVH exactly
// as render_view() does (src/main.cu:119-145,276), renders one frame with Render::run_view
// (src/main.cu:371-372) and saves it with Render::save_frame_buffer (src/main.cu:363).
// The GUI-settable knobs (spp, P_RR, light_sample_n, eye/lookat/up: Gui.h) are flags.
//
//   crt_cli <config.json> [-o out.png] [--spp N] [--p-rr X] [--lsn N] [--seed S] [--width W] [--height H]
//           [--eye x y z] [--lookat x y z] [--up x y z] [--reference | --exact | --fast] [--bounded-radiance] [--base-dir DIR] [--device N]
//           [--gpus N | --devices a,b,...] [--gather auto|rccl|copy] [--aov PREFIX] [--aov-specular PREFIX[,MAX_BOUNCES]]
//           [--denoise-specular] [--denoise PATH] [--denoise-iterations N] [--denoise-sigma c,n,a,d] [--denoise-variance] [--variance PATH]
//           [--denoise-nlm] [--denoise-nlm-params RADIUS,PATCH,K] [--denoise-regress] [--denoise-regress-params RADIUS,PATCH,K,RIDGE] [--denoise-scales N]
//           [--adaptive THRESHOLD] [--adaptive-min N] [--adaptive-step N] [--adaptive-samples PATH] [--adaptive-planned]
//           [--until THRESHOLD[,FRACTION[,MIN[,STEP]]]]
//           [--temporal N] [--temporal-step x,y,z] [--temporal-out PATH] [--temporal-denoise] [--temporal-clamp GAMMA[,RADIUS]]
//           [--temporal-variance samples|moments[,MIN_HISTORY]] [--temporal-specular [MIN_BOUNCES[,RADIUS[,MAX_BOUNCES]]]]
//           [--aov-shading PREFIX] [--demodulate] [--aov-direct PREFIX] [--aov-ao PREFIX[,SAMPLES[,DISTANCE]]]
//           [--upsample FACTOR[,RADIUS] --upsample-out PATH [--upsample-guide-spp N]] [--gathered PREFIX[,NAME,...]]
//           [--pixel-filter KIND[,RADIUS] --pixel-filter-out PATH]
// --pixel-filter KIND[,RADIUS] --pixel-filter-out PATH also writes the frame under a pixel reconstruction filter (one device;
// crt_set_pixel_filter, CRT_FLAG_PIXEL_FILTER, crt_filtered_frame): KIND is box, tent or mitchell, RADIUS defaults to 0.5, 1 and 2; every
// sample then counts for the pixels around its jittered position.  PATH gets a PNG, or with the ending .pfm the 3-channel mean.  -o stays
// the plain (box-filtered) frame of the same paths.  Not with --adaptive, --temporal or --gpus / --devices.
// --gathered PREFIX[,NAME,...] (only with --gpus / --devices) renders the frame with the buffers the image filters take gathered from all
// ranks (crt_multi_render_buffers) and writes each float plane asked for as PREFIX.<NAME>.pfm (3 channels; depth and coverage: 1): NAME
// is mean, variance, half_a, half_b, albedo, normal, depth, coverage, emission or diffuse_albedo; the default is mean, variance, albedo,
// normal, depth.  Every file holds the floats the single-device options write: --variance's, --aov's depth, --aov-shading's two.
// --upsample FACTOR[,RADIUS] --upsample-out PATH also renders the frame with resolution scaling (one device) and writes it as a PNG to PATH:
// the paths at (W / FACTOR, H / FACTOR), the shading AOVs with albedo, normal and depth at that size and at (W, H) -- there with
// --upsample-guide-spp samples per pixel (default: --spp) --, the low frame demodulated, upsampled along the two sets of guides
// (crt_upsample, its defaults; RADIUS 1 .. 4) and modulated with the full-resolution buffers.  FACTOR is 2 .. 8 and must divide --width and
// --height.  -o stays the plain frame at full size.  It runs last: --aov and --aov-shading write the buffers of the plain frame.
// --aov-direct PREFIX writes the direct-light AOVs of the frame (crt_render_aov_direct, one device): PREFIX_direct.pfm, PREFIX_unshadowed.pfm,
// PREFIX_direct_variance.pfm (3 channels) and PREFIX_visibility.pfm (1 channel).
// --aov-ao PREFIX[,SAMPLES[,DISTANCE]] writes the ambient-occlusion AOVs of the frame (crt_render_aov_ao, one device): PREFIX_ao.pfm,
// PREFIX_openness.pfm (1 channel) and PREFIX_bent.pfm (3 channels); SAMPLES 1 .. 256 rays per hit of at most DISTANCE > 0, either
// left out: crt_aov_ao_defaults'.
// --aov-shading PREFIX writes the shading AOVs of the frame (crt_render_aov_shading, one device, the trace of --aov): PREFIX.emission.pfm
// and PREFIX.diffuse_albedo.pfm (3 channels).  --demodulate makes --denoise and --temporal work on irradiance: the frame (and its
// variance) goes through crt_demodulate with those two buffers before the filter or the blend and the result through crt_modulate, so
// --temporal's history holds irradiance and --temporal-out is modulated with the last frame's buffers.
// --temporal N renders N frames on one device and accumulates them over time (crt_temporal, its defaults): frame f = 0 .. N-1 has eye and
// lookat moved by f x the --temporal-step vector and the seed --seed + f.  -o gets the last frame as rendered, --temporal-out PATH the
// accumulated last frame; --temporal-denoise writes the variance-guided filter (crt_denoise_var, its defaults with the --denoise-iterations
// / --denoise-sigma overrides) of the accumulated frame and its accumulated variance to --temporal-out instead.  --variance, --denoise and
// --aov work on the last frame as rendered.  --temporal-clamp GAMMA[,RADIUS] clamps the history to mean +- GAMMA deviations of the
// (2 RADIUS + 1)^2 current pixels around each pixel (crt_temporal_clamped; RADIUS 1 .. 3, default: crt_temporal_clamp_defaults').
// --temporal-specular [MIN_BOUNCES[,RADIUS[,MAX_BOUNCES]]] also reprojects what mirrors show through its virtual image (crt_temporal_dual:
// each frame runs the specular AOV pass with MAX_BOUNCES, default crt_aov_specular_defaults'; MIN_BOUNCES > 0 and RADIUS 1 .. 3 default
// to crt_temporal_dual_defaults'); it composes with --temporal-clamp, --temporal-denoise and --demodulate, not with --temporal-variance moments.
// --temporal-variance moments[,MIN_HISTORY] measures the variance --temporal-denoise filters with from the temporal moments of each pixel
// (crt_temporal_moments, crt_variance_estimate with its defaults, of_mean 1 and MIN_HISTORY) instead of carrying the per-sample variance
// along: the frames are then rendered without CRT_FLAG_VARIANCE and --spp 1 works.  samples (the default) is the carried variance.
// --adaptive THRESHOLD renders the frame with variance-driven adaptive sampling (crt_render_adaptive, one device): --spp is the cap, a
// pixel stops once the standard error of its mean is at most THRESHOLD x (mean + floor); --adaptive-min / --adaptive-step override the
// warm-up and the samples per pass of crt_adaptive_defaults, --adaptive-samples PATH writes the samples per pixel as a 1-channel PFM.
// --variance, --denoise and --aov work on the adaptive frame as on the uniform one.  --adaptive-planned renders it in two launches
// instead (crt_render_planned): the warm-up, then every pixel's remaining samples as planned from the warm-up's variance; --adaptive-step
// does not apply.
// --until THRESHOLD[,FRACTION[,MIN[,STEP]]] renders the uniform frame until it is clean enough (crt_render_until, one device): MIN
// samples of every pixel, then STEP more per range (crt_until_defaults' where not given) until at most FRACTION of the pixels (default
// 0) have a standard error above THRESHOLD x (mean + floor), or all --spp samples are in.  Prints the samples done and the last summary
// (crt_frame_error_info); the frame written is the preview at the samples done.  --variance, --denoise and --aov work on it as on the
// uniform frame.  Not with --adaptive, --temporal, --upsample, --pixel-filter, --denoise-select or --gpus / --devices.
// --variance PATH renders with CRT_FLAG_VARIANCE (the frame is the same bits) and writes the per-pixel variance of the mean
// (crt_variance, one device) as a 3-channel PFM.  --denoise-variance makes --denoise use the variance-guided filter (crt_denoise_var,
// its own defaults; --denoise-iterations / --denoise-sigma override them as well).  --denoise-nlm makes --denoise use the non-local-means
// filter (crt_denoise_nlm, its own defaults); --denoise-nlm-params sets its radius, patch and k, --denoise-sigma its three guide sigmas (the
// colour value is ignored: the filter has no colour sigma).  Not with --denoise-variance or --denoise-iterations.
// --denoise-regress makes --denoise use the first-order feature-regression filter (crt_denoise_regress, its own defaults, every feature;
// with --demodulate without the albedo feature); --denoise-regress-params sets its radius, patch, k and ridge, --denoise-sigma the scales
// of its normal, albedo and depth features.  Not with --denoise-nlm, --denoise-variance or --denoise-iterations.
// --denoise-scales N (1 .. 4) runs the filter of --denoise-variance, --denoise-nlm or --denoise-regress at N scales of a Laplacian pyramid
// (crt_pyramid_down, crt_pyramid_merge; Render::set_denoise_scales), with the same settings at every scale; it needs one of the three and
// is not for --denoise-select.
// --denoise-select LIST[,ERROR_RADIUS[,BLEND_RADIUS]] makes --denoise pick, per pixel, the one of the filters in LIST -- none, atrous, var,
// nlm, reg, joined by + (1 .. 4 of them), each with its own defaults, reg with its weights from the other half frame -- whose error estimated against the other half frame is smallest
// (CRT_FLAG_HALF_BUFFERS, crt_half_buffers, crt_filter_select; the radii default to crt_filter_select_defaults').  --denoise-choice PATH
// writes the choice map as a PNG (candidate k of K as the grey 255 k / max(K - 1, 1)).  Not with the other --denoise-* options or --demodulate.
// --denoise PATH renders as usual, then filters the frame with the AOV-guided a-trous denoiser (crt_denoise, one device) and writes the
// result as a PNG to PATH; -o and --aov outputs are unchanged by it.  --denoise-iterations (1 .. 5) and --denoise-sigma (colour, normal,
// albedo, depth) override crt_denoise_defaults.
// --aov PREFIX also writes the first-hit AOVs of the frame (crt_render_aov, one device): PREFIX_albedo.png (8-bit, 255 x clamp(a, 0, 1)
// truncated, no gamma), PREFIX_normal.png (255 x clamp((n + 1) / 2, 0, 1)) and PREFIX_depth.pfm (floats).
// --aov-specular PREFIX[,MAX_BOUNCES] writes the AOVs that follow mirror bounces (crt_render_aov_specular, one device; MAX_BOUNCES 1 .. 8,
// default: crt_aov_specular_defaults') as PFM files: PREFIX_guide_albedo.pfm and PREFIX_last_normal.pfm (3 channels), PREFIX_path_depth.pfm
// and PREFIX_bounces.pfm (1 channel).  --denoise-specular makes --denoise take guide_albedo of that pass (MAX_BOUNCES of --aov-specular if
// given) as its albedo guide instead of the first-hit albedo; normal and depth stay first-hit.
// --gpus N renders on devices 0..N-1 of this node in one process (crt_multi: interleaved pixel tiles, one RCCL all-gather);
// --devices names the device of every rank explicitly (a repeated index puts two ranks on one GPU: --gather copy only).
#include "crt_host.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <config.json> [-o out.png] [--spp N] [--p-rr X] [--lsn N] [--seed S] [--width W] [--height H]\n"
                             "       [--move-object INDEX,dx,dy,dz]...  (translates one object and refits the scene handle, once per use, before the frame)\n"
                             "       [--eye x y z] [--lookat x y z] [--up x y z] [--reference | --exact | --fast] [--bounded-radiance] [--base-dir DIR] [--device N]\n"
                             "       [--gpus N | --devices a,b,...] [--gather auto|rccl|copy] [--aov PREFIX] [--aov-specular PREFIX[,MAX_BOUNCES]]\n"
                             "       [--denoise-specular] [--aov-shading PREFIX] [--demodulate] [--aov-direct PREFIX]\n"
                             "       [--aov-ao PREFIX[,SAMPLES[,DISTANCE]]]\n"
                             "       [--denoise PATH] [--denoise-iterations N] [--denoise-sigma c,n,a,d] [--denoise-variance] [--variance PATH]\n"
                             "       [--denoise-nlm] [--denoise-nlm-params RADIUS,PATCH,K]  (--denoise-sigma: its colour value is ignored with --denoise-nlm)\n"
                             "       [--denoise-regress] [--denoise-regress-params RADIUS,PATCH,K,RIDGE]\n"
                             "       [--denoise-scales N]  (1 .. 4 scales of a pyramid over --denoise-variance, --denoise-nlm or --denoise-regress)\n"
                             "       [--denoise-select LIST[,ERROR_RADIUS[,BLEND_RADIUS]]] [--denoise-choice PATH]  (LIST: none, atrous, var, nlm, reg joined by +)\n"
                             "       [--adaptive THRESHOLD] [--adaptive-min N] [--adaptive-step N] [--adaptive-samples PATH] [--adaptive-planned]\n"
                             "       [--until THRESHOLD[,FRACTION[,MIN[,STEP]]]]\n"
                             "       [--temporal N] [--temporal-step x,y,z] [--temporal-out PATH] [--temporal-denoise] [--temporal-clamp GAMMA[,RADIUS]]\n"
                             "       [--temporal-variance samples|moments[,MIN_HISTORY]] [--temporal-specular [MIN_BOUNCES[,RADIUS[,MAX_BOUNCES]]]]\n"
                             "       [--upsample FACTOR[,RADIUS] --upsample-out PATH [--upsample-guide-spp N]]  (FACTOR 2 .. 8 divides --width and --height)\n"
                             "       [--pixel-filter KIND[,RADIUS] --pixel-filter-out PATH]  (KIND: box, tent, mitchell)\n"
                             "       [--gathered PREFIX[,NAME,...]]  (with --gpus / --devices; NAME: mean, variance, half_a, half_b, albedo, normal, depth, coverage,\n"
                             "                                        emission, diffuse_albedo; default: mean, variance, albedo, normal, depth)\n", argv[0]);
        return 2;
    }
    try {
        crt::TaskObjs all_objs;
        crt_task task = crt::load_task(argv[1], &all_objs);
        std::string out = "out.png", base_dir = ".", aov, aov_specular, aov_shading, aov_direct, aov_ao, denoise, variance, adaptive_samples, pixel_filter_out;
        crt_pixel_filter pixel_filter; // --pixel-filter
        bool pixel_filter_on = false;
        bool demodulate = false;
        crt_adaptive_params ad;
        crt_adaptive_defaults(&ad);
        bool adaptive = false, ad_option = false, planned = false;
        crt_until_params un;
        crt_until_defaults(&un);
        bool until = false;
        double until_fraction = 0.0;
        crt_denoise_params dn; // the overrides: 0 = take the default of the filter chosen
        std::memset(&dn, 0, sizeof(dn));
        bool dn_iterations = false, dn_sigma = false, denoise_var = false, denoise_specular = false;
        bool denoise_nlm = false, nlm_params = false;
        crt_nlm_params nlm; // --denoise-nlm: the filter's defaults with the overrides
        crt_denoise_nlm_defaults(&nlm);
        bool denoise_regress = false, regress_params = false;
        long denoise_scales = 0; // --denoise-scales N; 0: not given
        crt_regress_params reg; // --denoise-regress: the filter's defaults with the overrides
        crt_denoise_regress_defaults(&reg);
        std::vector<int> select_candidates; // --denoise-select: crt::Render::SELECT_* of LIST
        crt_filter_select_params sel;       // ... and the selection's defaults with the radii given
        crt_filter_select_defaults(&sel);
        std::string denoise_choice;
        uint32_t specular_bounces = 0; // 0: crt_aov_specular_defaults'
        uint32_t ao_samples = 0;       // --aov-ao; 0: crt_aov_ao_defaults', as is a distance of 0
        float ao_distance = 0.0f;
        int temporal = 0;
        bool temporal_option = false, temporal_denoise = false, temporal_clamp = false, temporal_moments = false;
        crt_variance_estimate_params tvar; // --temporal-variance moments: the estimate's defaults with of_mean 1 and MIN_HISTORY
        crt_variance_estimate_defaults(&tvar);
        tvar.of_mean = 1; // (the variance of the accumulated mean, which is what the filter is handed: docs/experiments.md)
        crt_temporal_clamp tclamp;
        crt_temporal_clamp_defaults(&tclamp);
        bool temporal_specular = false;
        crt_temporal_dual_params tdual;
        crt_temporal_dual_defaults(&tdual);
        uint32_t temporal_max_bounces = 0; // 0: crt_aov_specular_defaults'
        float temporal_step[3] = {0.0f, 0.0f, 0.0f};
        std::string temporal_out;
        unsigned upsample = 0, upsample_guide_spp = 0; // --upsample: the factor; 0 samples = the frame's
        bool upsample_option = false;
        crt_upsample_params up; // the operation's defaults with RADIUS
        crt_upsample_defaults(&up);
        std::string upsample_out;
        uint64_t seed = 0;
        int device = 0;
        bool reference = false, exact = false, fast = false, bounded = false;
        std::vector<int> devices;
        uint32_t gather = CRT_GATHER_AUTO;
        // --gathered: the float planes of crt_multi_buffers by name, the prefix, and the planes asked for in the order given
        const struct { const char* name; uint32_t bit, channels; } gathered_planes[] = {
            {"mean", CRT_MULTI_MEAN, 3}, {"variance", CRT_MULTI_VARIANCE, 3}, {"half_a", CRT_MULTI_HALF_A, 3}, {"half_b", CRT_MULTI_HALF_B, 3},
            {"albedo", CRT_MULTI_ALBEDO, 3}, {"normal", CRT_MULTI_NORMAL, 3}, {"depth", CRT_MULTI_DEPTH, 1}, {"coverage", CRT_MULTI_COVERAGE, 1},
            {"emission", CRT_MULTI_EMISSION, 3}, {"diffuse_albedo", CRT_MULTI_DIFFUSE_ALBEDO, 3}};
        std::string gathered;
        std::vector<size_t> gathered_rows;
        struct MoveObject { uint32_t index; float d[3]; };
        std::vector<MoveObject> moves; // --move-object, in the order given
        auto need = [&](int i, int n) { if (i + n >= argc) throw crt::Error(CRT_ERR_INVALID_ARG, std::string("missing value after ") + argv[i]); };
        for (int i = 2; i < argc; i++) {
            std::string a = argv[i];
            if (a == "-o") { need(i, 1); out = argv[++i]; }
            else if (a == "--spp") { need(i, 1); task.spp = (uint32_t)std::atoi(argv[++i]); }
            else if (a == "--p-rr") { need(i, 1); task.p_rr = (float)std::atof(argv[++i]); }
            else if (a == "--lsn") { need(i, 1); task.light_sample_n = (uint32_t)std::atoi(argv[++i]); }
            else if (a == "--seed") { need(i, 1); seed = std::strtoull(argv[++i], nullptr, 10); }
            else if (a == "--width") { need(i, 1); task.width = (uint32_t)std::atoi(argv[++i]); }
            else if (a == "--height") { need(i, 1); task.height = (uint32_t)std::atoi(argv[++i]); }
            else if (a == "--device") { need(i, 1); device = std::atoi(argv[++i]); }
            else if (a == "--gpus") {
                need(i, 1);
                const int n = std::atoi(argv[++i]);
                if (n < 1) throw crt::Error(CRT_ERR_INVALID_ARG, "--gpus needs a positive count");
                devices.clear();
                for (int k = 0; k < n; k++) devices.push_back(k);
            } else if (a == "--devices") {
                need(i, 1);
                devices.clear();
                for (const char* q = argv[++i]; *q;) {
                    char* end = nullptr;
                    const long v = std::strtol(q, &end, 10);
                    if (end == q) throw crt::Error(CRT_ERR_INVALID_ARG, "--devices needs a comma-separated list of device indices");
                    devices.push_back((int)v);
                    q = *end == ',' ? end + 1 : end;
                }
            } else if (a == "--gather") {
                need(i, 1);
                const std::string g = argv[++i];
                if (g == "auto") gather = CRT_GATHER_AUTO; else if (g == "rccl") gather = CRT_GATHER_RCCL; else if (g == "copy") gather = CRT_GATHER_COPY;
                else throw crt::Error(CRT_ERR_INVALID_ARG, "--gather must be auto, rccl or copy");
            }
            else if (a == "--gathered") {
                need(i, 1);
                const std::string v = argv[++i];
                size_t at = std::min(v.find(','), v.size());
                gathered = v.substr(0, at);
                if (gathered.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--gathered needs a PREFIX");
                gathered_rows.clear();
                while (at < v.size()) {
                    const size_t end = std::min(v.find(',', at + 1), v.size());
                    const std::string name = v.substr(at + 1, end - at - 1);
                    size_t row = 0;
                    while (row < sizeof(gathered_planes) / sizeof(gathered_planes[0]) && name != gathered_planes[row].name) row++;
                    if (row == sizeof(gathered_planes) / sizeof(gathered_planes[0]))
                        throw crt::Error(CRT_ERR_INVALID_ARG, "--gathered PREFIX[,NAME,...]: NAME is mean, variance, half_a, half_b, albedo, normal, depth, coverage, emission or diffuse_albedo, not '" + name + "'");
                    gathered_rows.push_back(row);
                    at = end;
                }
                if (gathered_rows.empty()) gathered_rows = {0, 1, 4, 5, 6}; // mean, variance, albedo, normal, depth
            }
            else if (a == "--base-dir") { need(i, 1); base_dir = argv[++i]; }
            else if (a == "--aov") { need(i, 1); aov = argv[++i]; }
            else if (a == "--aov-specular") {
                need(i, 1);
                aov_specular = argv[++i];
                const size_t comma = aov_specular.rfind(',');
                if (comma != std::string::npos) {
                    const int b = std::atoi(aov_specular.c_str() + comma + 1);
                    if (b < 1 || b > 8) throw crt::Error(CRT_ERR_INVALID_ARG, "--aov-specular PREFIX[,MAX_BOUNCES] needs MAX_BOUNCES in 1 .. 8");
                    specular_bounces = (uint32_t)b;
                    aov_specular.resize(comma);
                }
                if (aov_specular.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--aov-specular needs a PREFIX");
            }
            else if (a == "--aov-direct") { need(i, 1); aov_direct = argv[++i]; if (aov_direct.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--aov-direct needs a PREFIX"); }
            else if (a == "--aov-ao") {
                need(i, 1);
                aov_ao = argv[++i];
                const size_t c1 = aov_ao.find(',');
                if (c1 != std::string::npos) {
                    const std::string rest = aov_ao.substr(c1 + 1);
                    aov_ao.resize(c1);
                    const size_t c2 = rest.find(',');
                    const int n = std::atoi(rest.substr(0, c2).c_str());
                    if (n < 1 || n > 256) throw crt::Error(CRT_ERR_INVALID_ARG, "--aov-ao PREFIX[,SAMPLES[,DISTANCE]] needs SAMPLES in 1 .. 256");
                    ao_samples = (uint32_t)n;
                    if (c2 != std::string::npos) {
                        ao_distance = (float)std::atof(rest.c_str() + c2 + 1);
                        if (!(ao_distance > 0.0f && ao_distance <= 3.402823466e38f)) throw crt::Error(CRT_ERR_INVALID_ARG, "--aov-ao PREFIX[,SAMPLES[,DISTANCE]] needs a finite DISTANCE > 0");
                    }
                }
                if (aov_ao.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--aov-ao needs a PREFIX");
            }
            else if (a == "--aov-shading") { need(i, 1); aov_shading = argv[++i]; if (aov_shading.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--aov-shading needs a PREFIX"); }
            else if (a == "--demodulate") demodulate = true;
            else if (a == "--upsample") {
                need(i, 1);
                const char* q = argv[++i];
                char* end = nullptr;
                const long f = std::strtol(q, &end, 10);
                long r = 1;
                bool good = end != q && (*end == 0 || *end == ',');
                if (good && *end == ',') {
                    q = end + 1;
                    r = std::strtol(q, &end, 10);
                    good = end != q && *end == 0;
                }
                if (!good || f < 2 || f > 8 || r < 1 || r > 4) throw crt::Error(CRT_ERR_INVALID_ARG, "--upsample needs FACTOR[,RADIUS] with FACTOR 2 .. 8 and RADIUS 1 .. 4");
                upsample = (unsigned)f; up.radius = (uint32_t)r;
            }
            else if (a == "--upsample-out") { need(i, 1); upsample_out = argv[++i]; upsample_option = true; }
            else if (a == "--upsample-guide-spp") {
                need(i, 1);
                const int n = std::atoi(argv[++i]);
                if (n < 1) throw crt::Error(CRT_ERR_INVALID_ARG, "--upsample-guide-spp needs a positive count");
                upsample_guide_spp = (unsigned)n; upsample_option = true;
            }
            else if (a == "--denoise-specular") denoise_specular = true;
            else if (a == "--denoise") { need(i, 1); denoise = argv[++i]; }
            else if (a == "--denoise-variance") denoise_var = true;
            else if (a == "--denoise-nlm") denoise_nlm = true;
            else if (a == "--denoise-nlm-params") {
                need(i, 1);
                nlm_params = true;
                const char* q = argv[++i];
                char* end = nullptr;
                const long radius = std::strtol(q, &end, 10);
                bool good = end != q && *end == ',';
                long patch = 0;
                if (good) { q = end + 1; patch = std::strtol(q, &end, 10); good = end != q && *end == ','; }
                if (good) { q = end + 1; nlm.k = std::strtof(q, &end); good = end != q && *end == 0; }
                if (!good || radius < 0 || patch < 0) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-nlm-params needs three comma-separated values: RADIUS,PATCH,K");
                nlm.radius = (uint32_t)radius; nlm.patch = (uint32_t)patch;
            }
            else if (a == "--denoise-regress") denoise_regress = true;
            else if (a == "--denoise-regress-params") {
                need(i, 1);
                regress_params = true;
                const char* q = argv[++i];
                char* end = nullptr;
                const long radius = std::strtol(q, &end, 10);
                bool good = end != q && *end == ',';
                long patch = 0;
                if (good) { q = end + 1; patch = std::strtol(q, &end, 10); good = end != q && *end == ','; }
                if (good) { q = end + 1; reg.k = std::strtof(q, &end); good = end != q && *end == ','; }
                if (good) { q = end + 1; reg.ridge = std::strtof(q, &end); good = end != q && *end == 0; }
                if (!good || radius < 0 || patch < 0) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-regress-params needs four comma-separated values: RADIUS,PATCH,K,RIDGE");
                reg.radius = (uint32_t)radius; reg.patch = (uint32_t)patch;
            }
            else if (a == "--denoise-scales") {
                need(i, 1);
                char* end = nullptr;
                const char* q = argv[++i];
                denoise_scales = std::strtol(q, &end, 10);
                if (end == q || *end != 0 || denoise_scales < 1 || denoise_scales > 4) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-scales needs a number of scales 1 .. 4");
            }
            else if (a == "--variance") { need(i, 1); variance = argv[++i]; }
            else if (a == "--pixel-filter-out") { need(i, 1); pixel_filter_out = argv[++i]; }
            else if (a == "--pixel-filter") {
                need(i, 1);
                const std::string v = argv[++i];
                const size_t comma = v.find(',');
                const std::string kind = v.substr(0, comma);
                bool good = kind == "box" || kind == "tent" || kind == "mitchell";
                pixel_filter.kind = kind == "box" ? CRT_PIXEL_FILTER_BOX : kind == "tent" ? CRT_PIXEL_FILTER_TENT : CRT_PIXEL_FILTER_MITCHELL;
                pixel_filter.radius = kind == "box" ? 0.5f : kind == "tent" ? 1.0f : 2.0f;
                if (good && comma != std::string::npos) {
                    const char* q = v.c_str() + comma + 1;
                    char* end = nullptr;
                    pixel_filter.radius = std::strtof(q, &end);
                    good = end != q && *end == 0;
                }
                if (!good) throw crt::Error(CRT_ERR_INVALID_ARG, "--pixel-filter needs KIND[,RADIUS]: KIND box, tent or mitchell");
                pixel_filter_on = true;
            }
            else if (a == "--adaptive") { need(i, 1); ad.threshold = std::strtof(argv[++i], nullptr); adaptive = true; }
            else if (a == "--adaptive-min") { need(i, 1); ad.min_samples = (uint32_t)std::atoi(argv[++i]); ad_option = true; }
            else if (a == "--adaptive-step") { need(i, 1); ad.step_samples = (uint32_t)std::atoi(argv[++i]); ad_option = true; }
            else if (a == "--adaptive-samples") { need(i, 1); adaptive_samples = argv[++i]; ad_option = true; }
            else if (a == "--adaptive-planned") { planned = true; ad_option = true; }
            else if (a == "--until") {
                need(i, 1);
                const char* q = argv[++i];
                char* end = nullptr;
                bool good = true;
                un.threshold = std::strtof(q, &end);
                good = end != q;
                if (good && *end == ',') { q = end + 1; until_fraction = std::strtod(q, &end); good = end != q && until_fraction >= 0.0 && until_fraction < 1.0; }
                if (good && *end == ',') { q = end + 1; const long n = std::strtol(q, &end, 10); good = end != q && n >= 2; un.min_samples = (uint32_t)n; }
                if (good && *end == ',') { q = end + 1; const long n = std::strtol(q, &end, 10); good = end != q && n >= 1; un.step_samples = (uint32_t)n; }
                if (!good || *end != 0) throw crt::Error(CRT_ERR_INVALID_ARG, "--until needs THRESHOLD[,FRACTION[,MIN[,STEP]]]: FRACTION in [0, 1), MIN >= 2, STEP >= 1");
                until = true;
            }
            else if (a == "--temporal") {
                need(i, 1);
                temporal = std::atoi(argv[++i]);
                if (temporal < 1) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal needs a positive number of frames");
            }
            else if (a == "--temporal-step") {
                need(i, 1);
                temporal_option = true;
                const char* q = argv[++i];
                for (int k = 0; k < 3; k++) {
                    char* end = nullptr;
                    temporal_step[k] = std::strtof(q, &end);
                    if (end == q || (k < 2 ? *end != ',' : *end != 0)) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal-step needs three comma-separated values: x,y,z");
                    q = end + 1;
                }
            }
            else if (a == "--temporal-out") { need(i, 1); temporal_out = argv[++i]; temporal_option = true; }
            else if (a == "--temporal-denoise") { temporal_denoise = true; temporal_option = true; }
            else if (a == "--temporal-clamp") {
                need(i, 1);
                temporal_clamp = temporal_option = true;
                const char* q = argv[++i];
                char* end = nullptr;
                tclamp.gamma = std::strtof(q, &end);
                bool good = end != q && (*end == 0 || *end == ',') && tclamp.gamma >= 0.0f; // (false for NaN)
                if (good && *end == ',') {
                    q = end + 1;
                    const long r = std::strtol(q, &end, 10);
                    good = end != q && *end == 0 && r >= 1 && r <= 3;
                    tclamp.radius = (uint32_t)r;
                }
                if (!good) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal-clamp needs GAMMA[,RADIUS]: GAMMA >= 0, RADIUS 1 .. 3");
            }
            else if (a == "--temporal-specular") {
                temporal_specular = temporal_option = true;
                // (the value is optional: the next argument is one unless it is another option; "-1" is a value, and a bad one)
                const char* nx = i + 1 < argc ? argv[i + 1] : nullptr;
                if (nx && (nx[0] != '-' || (nx[1] >= '0' && nx[1] <= '9') || nx[1] == '.')) {
                    const char* q = argv[++i];
                    char* end = nullptr;
                    tdual.min_bounces = std::strtof(q, &end);
                    bool good = end != q && (*end == 0 || *end == ',') && tdual.min_bounces > 0.0f; // (false for NaN)
                    if (good && *end == ',') {
                        q = end + 1;
                        const long r = std::strtol(q, &end, 10);
                        good = end != q && (*end == 0 || *end == ',') && r >= 1 && r <= 3;
                        tdual.radius = (uint32_t)r;
                        if (good && *end == ',') {
                            q = end + 1;
                            const long b = std::strtol(q, &end, 10);
                            good = end != q && *end == 0 && b >= 1 && b <= 8;
                            temporal_max_bounces = (uint32_t)b;
                        }
                    }
                    if (!good) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal-specular takes [MIN_BOUNCES[,RADIUS[,MAX_BOUNCES]]]: MIN_BOUNCES > 0, RADIUS 1 .. 3, MAX_BOUNCES 1 .. 8");
                }
            }
            else if (a == "--temporal-variance") {
                need(i, 1);
                temporal_option = true;
                const std::string v = argv[++i];
                bool good = true;
                if (v == "samples") temporal_moments = false;
                else if (v == "moments") temporal_moments = true;
                else if (v.rfind("moments,", 0) == 0) {
                    const char* q = v.c_str() + 8;
                    char* end = nullptr;
                    const long m = std::strtol(q, &end, 10);
                    good = *q >= '0' && *q <= '9' && *end == 0 && m >= 1 && m <= 1000000;
                    tvar.min_history = (uint32_t)m;
                    temporal_moments = true;
                } else good = false;
                if (!good) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal-variance needs samples or moments[,MIN_HISTORY]: MIN_HISTORY >= 1");
            }
            else if (a == "--denoise-choice") { need(i, 1); denoise_choice = argv[++i]; }
            else if (a == "--denoise-select") {
                need(i, 1);
                const std::string v = argv[++i];
                const size_t comma = v.find(',');
                const std::string list = v.substr(0, comma);
                bool good = !list.empty();
                for (size_t at = 0; good && at <= list.size();) {
                    const size_t plus = std::min(list.find('+', at), list.size());
                    const std::string name = list.substr(at, plus - at);
                    const int id = name == "none" ? crt::Render::SELECT_NONE : name == "atrous" ? crt::Render::SELECT_ATROUS : name == "var" ? crt::Render::SELECT_VAR
                                 : name == "nlm" ? crt::Render::SELECT_NLM : name == "reg" ? crt::Render::SELECT_REG : -1;
                    good = id >= 0 && select_candidates.size() < CRT_SELECT_MAX_CANDIDATES;
                    select_candidates.push_back(id);
                    at = plus + 1;
                }
                uint32_t* dst[2] = {&sel.error_radius, &sel.blend_radius};
                const char* q = comma == std::string::npos ? "" : v.c_str() + comma + 1;
                for (int k = 0; good && comma != std::string::npos && k < 2; k++) {
                    char* end = nullptr;
                    const long r = std::strtol(q, &end, 10);
                    good = *q >= '0' && *q <= '9' && (*end == 0 || (k == 0 && *end == ',')) && r <= (k == 0 ? 8 : 4);
                    *dst[k] = (uint32_t)r;
                    if (*end == 0) break;
                    q = end + 1;
                }
                if (!good) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-select needs LIST[,ERROR_RADIUS[,BLEND_RADIUS]]: LIST 1 .. 4 of none, atrous, var, nlm, reg joined by +, ERROR_RADIUS 0 .. 8, BLEND_RADIUS 0 .. 4");
            }
            else if (a == "--denoise-iterations") { need(i, 1); dn.iterations = (uint32_t)std::atoi(argv[++i]); dn_iterations = true; }
            else if (a == "--denoise-sigma") {
                need(i, 1);
                dn_sigma = true;
                float* dst[4] = {&dn.sigma_color, &dn.sigma_normal, &dn.sigma_albedo, &dn.sigma_depth};
                const char* q = argv[++i];
                for (int k = 0; k < 4; k++) {
                    char* end = nullptr;
                    *dst[k] = std::strtof(q, &end);
                    if (end == q || (k < 3 ? *end != ',' : *end != 0)) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-sigma needs four comma-separated values: colour,normal,albedo,depth");
                    q = end + 1;
                }
            }
            else if (a == "--move-object") {
                need(i, 1);
                const char* q = argv[++i];
                char* e = nullptr;
                MoveObject mo;
                mo.index = (uint32_t)std::strtoul(q, &e, 10);
                bool good = e != q;
                for (int k = 0; k < 3 && good; k++) {
                    good = *e == ',';
                    if (good) { q = e + 1; mo.d[k] = std::strtof(q, &e); good = e != q; }
                }
                if (!good || *e) throw crt::Error(CRT_ERR_INVALID_ARG, "--move-object needs INDEX,dx,dy,dz");
                moves.push_back(mo);
            }
            else if (a == "--reference") reference = true;
            else if (a == "--exact") exact = true;
            else if (a == "--fast") fast = true;
            else if (a == "--bounded-radiance") bounded = true; // CRT_FLAG_BOUNDED_RADIANCE: a ring of samples instead of one radiance per path
            else if (a == "--eye" || a == "--lookat" || a == "--up") {
                need(i, 3);
                float* dst = a == "--eye" ? task.eye_pos : (a == "--lookat" ? task.lookat : task.up);
                for (int k = 0; k < 3; k++) dst[k] = (float)std::atof(argv[++i]);
            } else throw crt::Error(CRT_ERR_INVALID_ARG, "unknown option " + a);
        }
        crt::Scene scene(task.width, task.height);
        crt::load_task_scene(task, scene, base_dir, &all_objs);
        scene.set_BVH(task.bvh_thresh_n);
        std::printf("triangles: %zu, BVH nodes: %zu, lights: %zu\n", scene.get_triangles().size(), scene.get_bvh().get_nodes_size(),
                    scene.get_light_objs().size());
        const bool multi = !devices.empty();
        // The options that work on one device.  The first refusal that applies is the one reported, so the rows stand in the order of
        // the refusals and refuse_on_many takes the next `count` of them where theirs stood among the other checks.
        const struct { bool present; const char* what; } one_device[] = {
            {!aov.empty(), "--aov renders on one device"}, {!aov_specular.empty(), "--aov-specular renders on one device"},
            {!aov_shading.empty(), "--aov-shading renders on one device"}, {!aov_direct.empty(), "--aov-direct renders on one device"}, {!aov_ao.empty(), "--aov-ao renders on one device"}, {!denoise.empty(), "--denoise filters on one device"},
            {!variance.empty(), "--variance reads one device's buffer"}, {denoise_var, "--denoise-variance filters on one device"},
            {adaptive, "--adaptive renders on one device"}, {temporal != 0, "--temporal accumulates on one device"}, {upsample != 0, "--upsample runs on one device"},
            {denoise_nlm, "--denoise-nlm filters on one device"}, {denoise_regress, "--denoise-regress filters on one device"}};
        size_t row = 0;
        auto refuse_on_many = [&](size_t count) {
            for (; count-- > 0; row++)
                if (multi && one_device[row].present) throw crt::Error(CRT_ERR_INVALID_ARG, std::string(one_device[row].what) + " (not with --gpus / --devices)");
        };
        refuse_on_many(5);
        if (demodulate && denoise.empty() && !temporal) throw crt::Error(CRT_ERR_INVALID_ARG, "--demodulate needs --denoise PATH or --temporal N");
        if (denoise_specular && denoise.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-specular needs --denoise PATH");
        refuse_on_many(6);
        if (upsample_option && !upsample) throw crt::Error(CRT_ERR_INVALID_ARG, "--upsample-out and --upsample-guide-spp need --upsample FACTOR");
        if (upsample && upsample_out.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--upsample needs --upsample-out PATH");
        if (upsample && (task.width % upsample || task.height % upsample))
            throw crt::Error(CRT_ERR_INVALID_ARG, "--upsample: FACTOR must divide --width and --height");
        if (adaptive && temporal) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal accumulates uniformly sampled frames (not with --adaptive)");
        if (temporal_option && !temporal) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal-step, --temporal-out, --temporal-denoise, --temporal-clamp, --temporal-variance and --temporal-specular need --temporal N");
        if (temporal_specular && temporal_moments) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal-specular cannot be combined with --temporal-variance moments (crt_temporal_moments has no dual form)");
        if (temporal_denoise && temporal_out.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--temporal-denoise needs --temporal-out PATH");
        if (until && multi) throw crt::Error(CRT_ERR_INVALID_ARG, "--until renders on one device (not with --gpus / --devices)");
        if (until && (adaptive || temporal || upsample || pixel_filter_on || !select_candidates.empty()))
            throw crt::Error(CRT_ERR_INVALID_ARG, "--until renders the uniformly sampled frame in ranges (not with --adaptive, --temporal, --upsample, --pixel-filter or --denoise-select)");
        if (ad_option && !adaptive) throw crt::Error(CRT_ERR_INVALID_ARG, "--adaptive-min, --adaptive-step, --adaptive-samples and --adaptive-planned need --adaptive THRESHOLD");
        if (denoise_var && denoise.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-variance needs --denoise PATH");
        // --denoise-nlm and --denoise-regress: filters of their own with the same rules; --denoise-sigma's guide sigmas go to their settings
        const struct { std::string flag; bool on, params, others; const char* not_with; float* sigmas[3]; } own_filters[] = {
            {"--denoise-nlm", denoise_nlm, nlm_params, denoise_var, "--denoise-variance", {&nlm.sigma_normal, &nlm.sigma_albedo, &nlm.sigma_depth}},
            {"--denoise-regress", denoise_regress, regress_params, denoise_var || denoise_nlm, "--denoise-variance or --denoise-nlm", {&reg.sigma_normal, &reg.sigma_albedo, &reg.sigma_depth}}};
        for (const auto& f : own_filters) {
            refuse_on_many(1);
            if (f.on && denoise.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, f.flag + " needs --denoise PATH");
            if (f.params && !f.on) throw crt::Error(CRT_ERR_INVALID_ARG, f.flag + "-params needs " + f.flag);
            if (f.on && f.others) throw crt::Error(CRT_ERR_INVALID_ARG, f.flag + " is a filter of its own (not with " + f.not_with + ")");
            if (f.on && dn_iterations) throw crt::Error(CRT_ERR_INVALID_ARG, f.flag + " is one pass (not with --denoise-iterations)");
            if (f.on && dn_sigma) { *f.sigmas[0] = dn.sigma_normal; *f.sigmas[1] = dn.sigma_albedo; *f.sigmas[2] = dn.sigma_depth; }
        }
        const bool denoise_select = !select_candidates.empty();
        if (denoise_select && denoise.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-select needs --denoise PATH");
        if (!denoise_choice.empty() && !denoise_select) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-choice needs --denoise-select LIST");
        if (denoise_select && (denoise_var || denoise_nlm || denoise_regress || dn_iterations || dn_sigma || denoise_specular || demodulate))
            throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-select runs every filter with its own defaults on radiance (not with the other --denoise-* options or --demodulate)");
        if (denoise_scales && denoise_select) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-scales is not for --denoise-select (the half frames are filtered at one scale)");
        if (denoise_scales && !(denoise_var || denoise_nlm || denoise_regress))
            throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-scales needs --denoise-variance, --denoise-nlm or --denoise-regress (the pyramid reduces the variance with the frame)");
        if (denoise_select && (adaptive || temporal)) throw crt::Error(CRT_ERR_INVALID_ARG, "--denoise-select needs the half buffers of a uniformly sampled frame (not with --adaptive or --temporal)");
        if (pixel_filter_on != !pixel_filter_out.empty()) throw crt::Error(CRT_ERR_INVALID_ARG, "--pixel-filter KIND[,RADIUS] and --pixel-filter-out PATH go together");
        if (pixel_filter_on && (multi || adaptive || temporal))
            throw crt::Error(CRT_ERR_INVALID_ARG, "--pixel-filter filters the uniformly sampled frame of one device (not with --gpus / --devices, --adaptive or --temporal)");
        if (!gathered.empty() && !multi) throw crt::Error(CRT_ERR_INVALID_ARG, "--gathered gathers the buffers of a multi-device frame (only with --gpus / --devices)");
        const bool want_var = !variance.empty() || denoise_var || denoise_nlm || denoise_regress || (temporal > 0 && !temporal_moments);
        crt_denoise_params tdn; // --temporal-denoise: the variance-guided filter's defaults with the overrides
        crt_denoise_var_defaults(&tdn);
        if (dn_iterations) tdn.iterations = dn.iterations;
        if (dn_sigma) { tdn.sigma_color = dn.sigma_color; tdn.sigma_normal = dn.sigma_normal; tdn.sigma_albedo = dn.sigma_albedo; tdn.sigma_depth = dn.sigma_depth; }
        {
            crt_denoise_params d;
            if (denoise_var) crt_denoise_var_defaults(&d); else crt_denoise_defaults(&d);
            if (dn_iterations) d.iterations = dn.iterations;
            if (dn_sigma) { d.sigma_color = dn.sigma_color; d.sigma_normal = dn.sigma_normal; d.sigma_albedo = dn.sigma_albedo; d.sigma_depth = dn.sigma_depth; }
            dn = d;
        }
        crt::Render render_one_or_many = multi ? crt::Render(&scene, task.spp, task.p_rr, task.light_sample_n, devices, gather)
                                               : crt::Render(&scene, task.spp, task.p_rr, task.light_sample_n, device);
        crt::Render& render = render_one_or_many;
        render.set_seed(seed);
        render.set_traversal(reference ? CRT_TRAVERSAL_REFERENCE : (fast && !exact) ? CRT_TRAVERSAL_FAST : CRT_TRAVERSAL_EXACT);
        render.set_flags((bounded ? CRT_FLAG_BOUNDED_RADIANCE : 0u) | (want_var ? CRT_FLAG_VARIANCE : 0u) | (denoise_select ? CRT_FLAG_HALF_BUFFERS : 0u) |
                         (pixel_filter_on ? CRT_FLAG_PIXEL_FILTER : 0u));
        if (pixel_filter_on) render.set_pixel_filter(&pixel_filter);
        if (!moves.empty() && multi) throw crt::Error(CRT_ERR_INVALID_ARG, "--move-object refits one device's scene handle (not with --gpus / --devices)");
        for (const MoveObject& mo : moves) { // the handle was made from the scene as loaded: each move is one refit of it
            const float m[12] = {1.0f, 0.0f, 0.0f, mo.d[0], 0.0f, 1.0f, 0.0f, mo.d[1], 0.0f, 0.0f, 1.0f, mo.d[2]};
            scene.transform_object(mo.index, m);
            const crt_refit_info ri = render.refit();
            std::printf("moved object %u by (%g, %g, %g): refit %.3f ms on the device (tables %.3f ms), %u launches\n", mo.index, mo.d[0], mo.d[1], mo.d[2], ri.device_ms,
                        ri.prepare_ms, ri.launches);
        }
        render.set_aov_shading(!aov_shading.empty());
        if (demodulate) render.set_demodulate(true);
        // One output's files -- a PFM of 1 or 3 channels of floats, or with channels 0 a PNG of RGB8 -- are written, then their paths printed
        struct OutFile { std::string path; uint32_t channels; const void* data; };
        auto write_files = [&](const char* what, std::initializer_list<OutFile> files) {
            for (const OutFile& f : files) {
                const int rc = f.channels ? crt_write_pfm(f.path.c_str(), task.width, task.height, f.channels, (const float*)f.data)
                                          : crt_write_png(f.path.c_str(), task.width, task.height, (const uint8_t*)f.data);
                if (rc != CRT_OK) throw crt::Error(rc, std::string("writing the ") + what + " failed: " + crt_last_error());
            }
            for (const OutFile& f : files) std::printf("%s\n", f.path.c_str());
        };
        float inv_view[9];
        crt::get_inverse_view_matrix(task.eye_pos, task.lookat, task.up, inv_view);
        float fov_y = task.fov_y * (float)M_PI / 180; // src/main.cu:278
        auto t0 = std::chrono::high_resolution_clock::now();
        if (temporal) {
            crt_temporal_params tp;
            crt_temporal_defaults(&tp);
            const float eye0[3] = {task.eye_pos[0], task.eye_pos[1], task.eye_pos[2]}, lookat0[3] = {task.lookat[0], task.lookat[1], task.lookat[2]};
            for (int f = 0; f < temporal; f++) { // (the last frame's camera stays in task / inv_view for the outputs below)
                for (int k = 0; k < 3; k++) {
                    task.eye_pos[k] = eye0[k] + (float)f * temporal_step[k];
                    task.lookat[k] = lookat0[k] + (float)f * temporal_step[k];
                }
                crt::get_inverse_view_matrix(task.eye_pos, task.lookat, task.up, inv_view);
                render.set_seed(seed + (uint64_t)f);
                if (temporal_moments) render.run_temporal_moments(task.eye_pos, inv_view, fov_y, tp, temporal_clamp ? &tclamp : nullptr, tvar);
                else if (temporal_specular) render.run_temporal_specular(task.eye_pos, inv_view, fov_y, tp, temporal_clamp ? &tclamp : nullptr, tdual, temporal_max_bounces);
                else render.run_temporal(task.eye_pos, inv_view, fov_y, tp, temporal_clamp ? &tclamp : nullptr);
                std::printf("temporal frame %d: %llu of %llu pixels reprojected, device %.3f ms\n", f, (unsigned long long)render.last_temporal_info().reprojected,
                            (unsigned long long)task.width * task.height, render.last_temporal_info().total_ms);
                if (temporal_clamp) std::printf("temporal frame %d: %llu histories clamped (gamma %g, radius %u)\n", f, (unsigned long long)render.last_temporal_clamped(),
                                                (double)tclamp.gamma, tclamp.radius);
                if (temporal_specular) std::printf("temporal frame %d: %llu pixels tried their virtual image, %llu took it (min_bounces %g, radius %u)\n", f,
                                                   (unsigned long long)render.last_temporal_dual_info().virtual_tried,
                                                   (unsigned long long)render.last_temporal_dual_info().virtual_taken, (double)tdual.min_bounces, tdual.radius);
                if (temporal_moments) std::printf("temporal frame %d: variance of %llu pixels from their neighbourhood (history below %u), device %.3f ms\n", f,
                                                  (unsigned long long)render.last_variance_estimate_info().spatial, tvar.min_history,
                                                  render.last_variance_estimate_info().total_ms);
            }
        }
        else if (adaptive && planned) render.run_view_planned(task.eye_pos, inv_view, fov_y, ad, want_var);
        else if (adaptive) render.run_view_adaptive(task.eye_pos, inv_view, fov_y, ad, want_var);
        else if (until) {
            un.max_above = (uint64_t)(until_fraction * (double)((uint64_t)task.width * task.height));
            render.run_view_until(task.eye_pos, inv_view, fov_y, un, 0, want_var);
        }
        else if (!gathered.empty()) {
            uint32_t want = 0;
            for (size_t r : gathered_rows) want |= gathered_planes[r].bit;
            render.run_view_gathered(task.eye_pos, inv_view, fov_y, want);
        }
        else render.run_view(task.eye_pos, inv_view, fov_y);
        std::chrono::duration<double> dt = std::chrono::high_resolution_clock::now() - t0;
        if (adaptive && planned) {
            const crt_map_info& mi = render.last_map_info();
            std::printf("render cost: %.6f seconds (device %.3f ms, planned: %u launches, %llu of %llu paths)\n", dt.count(), mi.total_ms, mi.launches,
                        (unsigned long long)mi.paths, (unsigned long long)mi.paths_uniform);
        } else if (until) {
            const crt_until_info& ui = render.last_until_info();
            const crt_frame_error_info& e = ui.last;
            std::printf("render cost: %.6f seconds (device %.3f ms, until: %u of %u samples in %u ranges, %u checks, %llu paths)\n", dt.count(), ui.total_ms,
                        ui.samples_done, e.spp, ui.passes, ui.checks, (unsigned long long)ui.paths);
            std::printf("until: %llu of %llu pixels above the target (%llu allowed, %llu NaN), sum_variance %.17g, sum_mean %.17g\nuntil: hist", (unsigned long long)e.above,
                        (unsigned long long)e.pixels, (unsigned long long)un.max_above, (unsigned long long)e.nan_pixels, e.sum_variance, e.sum_mean);
            for (int b = 0; b < 16; b++) std::printf(" %llu", (unsigned long long)e.hist[b]);
            std::printf("\n");
        } else if (adaptive) {
            const crt_adaptive_info& ai = render.last_adaptive_info();
            std::printf("render cost: %.6f seconds (device %.3f ms, adaptive: %u passes, %llu of %llu paths)\n", dt.count(), ai.total_ms, ai.passes,
                        (unsigned long long)ai.paths, (unsigned long long)ai.paths_uniform);
        } else {
            const crt_stats& st = render.last_stats();
            std::printf("render cost: %.6f seconds (device %.3f ms, %llu rays, %.1f Mrays/s)\n", dt.count(), st.total_ms,
                        (unsigned long long)st.rays, st.total_ms > 0 ? st.rays / st.total_ms / 1e3 : 0.0);
        }
        if (multi) {
            const crt_multi_info& mi = render.last_multi_info();
            std::printf("ranks: %u, gather: %s, rccl ranks: %u (rccl %d), %llu B per rank, render %.3f ms + gather %.3f ms\n", mi.n_ranks,
                        mi.gather == CRT_GATHER_RCCL ? "rccl" : "copy", mi.rccl_ranks, mi.rccl_version, (unsigned long long)mi.bytes_per_rank,
                        mi.render_ms, mi.gather_ms);
            if (mi.fallback_reason[0]) std::printf("gather fell back to peer copies: %s\n", mi.fallback_reason);
        }
        render.save_frame_buffer(out.c_str());
        std::printf("%s\n", out.c_str());
        for (size_t r : gathered_rows) // (one at a time: their number is the caller's)
            write_files("gathered plane", {{gathered + "." + gathered_planes[r].name + ".pfm", gathered_planes[r].channels, render.get_gathered_buffer(gathered_planes[r].bit)}});
        if (!variance.empty()) write_files("variance file", {{variance, 3, render.variance()}});
        if (pixel_filter_on) { // (before the calls below that render again: it reads the sums of the frame just rendered)
            render.filtered_frame();
            const bool pfm = pixel_filter_out.size() >= 4 && pixel_filter_out.compare(pixel_filter_out.size() - 4, 4, ".pfm") == 0;
            if (pfm) write_files("filtered frame", {{pixel_filter_out, 3, render.get_filtered_mean_buffer()}});
            else { render.save_filtered_buffer(pixel_filter_out.c_str()); std::printf("%s\n", pixel_filter_out.c_str()); }
        }
        if (!adaptive_samples.empty()) {
            std::vector<float> ns((size_t)task.width * task.height);
            for (size_t k = 0; k < ns.size(); k++) ns[k] = (float)render.get_samples_buffer()[k];
            write_files("samples file", {{adaptive_samples, 1, ns.data()}});
        }
        if (!aov.empty() || !aov_shading.empty() || !denoise.empty()) render.run_aov(task.eye_pos, inv_view, fov_y);
        if (!aov_shading.empty()) {
            const crt_aov_info& ai = render.last_aov_info();
            std::printf("aov-shading: %llu rays in %u chunks, device %.3f ms\n", (unsigned long long)ai.rays, ai.chunks, ai.total_ms);
            write_files("shading AOV files", {{aov_shading + ".emission.pfm", 3, render.get_emission_buffer()}, {aov_shading + ".diffuse_albedo.pfm", 3, render.get_diffuse_albedo_buffer()}});
        }
        if (!aov.empty()) {
            const crt_aov_info& ai = render.last_aov_info();
            std::printf("aov: %llu rays in %u chunks, device %.3f ms\n", (unsigned long long)ai.rays, ai.chunks, ai.total_ms);
            const size_t n = (size_t)task.width * task.height;
            // (float arithmetic throughout; to_u8 truncates as the frame's tone map does)
            auto to_u8 = [](float v) -> uint8_t { return !(v == v) || v <= 0.0f ? 0 : v >= 255.0f ? 255 : (uint8_t)v; };
            auto unit_clamp = [](float v) { return v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v; };
            std::vector<uint8_t> albedo(3 * n), normal(3 * n);
            for (size_t k = 0; k < 3 * n; k++) {
                albedo[k] = to_u8(255.0f * unit_clamp(render.get_albedo_buffer()[k]));
                normal[k] = to_u8(255.0f * unit_clamp((render.get_normal_buffer()[k] + 1.0f) / 2.0f));
            }
            write_files("AOV files", {{aov + "_albedo.png", 0, albedo.data()}, {aov + "_normal.png", 0, normal.data()}, {aov + "_depth.pfm", 1, render.get_depth_buffer()}});
        }
        if (!aov_direct.empty()) {
            render.run_view_aov_direct(task.eye_pos, inv_view, fov_y);
            const crt_aov_info& ai = render.last_aov_direct_info();
            std::printf("aov-direct: %llu rays in %u sub-batches, device %.3f ms\n", (unsigned long long)ai.rays, ai.chunks, ai.total_ms);
            write_files("direct-light AOV files", {{aov_direct + "_direct.pfm", 3, render.get_direct_buffer()}, {aov_direct + "_unshadowed.pfm", 3, render.get_unshadowed_buffer()},
                                                   {aov_direct + "_direct_variance.pfm", 3, render.get_direct_variance_buffer()},
                                                   {aov_direct + "_visibility.pfm", 1, render.get_visibility_buffer()}});
        }
        if (!aov_ao.empty()) {
            render.run_view_aov_ao(task.eye_pos, inv_view, fov_y, ao_samples, ao_distance);
            const crt_aov_info& ai = render.last_aov_ao_info();
            std::printf("aov-ao: %llu rays in %u sub-batches, device %.3f ms\n", (unsigned long long)ai.rays, ai.chunks, ai.total_ms);
            write_files("ambient-occlusion AOV files", {{aov_ao + "_ao.pfm", 1, render.get_ao_buffer()}, {aov_ao + "_openness.pfm", 1, render.get_openness_buffer()},
                                                        {aov_ao + "_bent.pfm", 3, render.get_bent_normal_buffer()}});
        }
        if (!aov_specular.empty() || denoise_specular) { // (after --aov's files: as the guide it replaces the first-hit albedo)
            render.run_aov_specular(task.eye_pos, inv_view, fov_y, specular_bounces, denoise_specular);
            const crt_aov_info& ai = render.last_aov_specular_info();
            std::printf("aov-specular: %llu rays in %u chunks, device %.3f ms\n", (unsigned long long)ai.rays, ai.chunks, ai.total_ms);
        }
        if (!aov_specular.empty())
            write_files("specular AOV files", {{aov_specular + "_guide_albedo.pfm", 3, render.get_guide_albedo_buffer()}, {aov_specular + "_last_normal.pfm", 3, render.get_last_normal_buffer()},
                                               {aov_specular + "_path_depth.pfm", 1, render.get_path_depth_buffer()}, {aov_specular + "_bounces.pfm", 1, render.get_bounces_buffer()}});
        if (denoise_select) {
            render.run_denoise_select(select_candidates, sel);
            const crt_filter_select_info& si = render.last_select_info();
            std::printf("denoise-select: error radius %u, blend radius %u, pixels per candidate %llu %llu %llu %llu, device %.3f ms\n", sel.error_radius, sel.blend_radius,
                        (unsigned long long)si.chosen[0], (unsigned long long)si.chosen[1], (unsigned long long)si.chosen[2], (unsigned long long)si.chosen[3], si.total_ms);
            render.save_denoised_buffer(denoise.c_str());
            std::printf("%s\n", denoise.c_str());
            if (!denoise_choice.empty()) {
                const size_t n = (size_t)task.width * task.height, top = select_candidates.size() > 1 ? select_candidates.size() - 1 : 1;
                std::vector<uint8_t> grey(3 * n);
                for (size_t k = 0; k < n; k++) grey[3 * k] = grey[3 * k + 1] = grey[3 * k + 2] = (uint8_t)(255u * render.get_choice_buffer()[k] / top);
                write_files("choice map", {{denoise_choice, 0, grey.data()}});
            }
        } else if (!denoise.empty()) {
            if (denoise_scales) render.set_denoise_scales((unsigned)denoise_scales);
            if (denoise_regress) render.run_denoise_regress(reg); else if (denoise_nlm) render.run_denoise_nlm(nlm); else if (denoise_var) render.run_denoise_var(dn); else render.run_denoise(dn);
            const crt_denoise_info& di = render.last_denoise_info();
            std::printf("denoise: %u passes, device %.3f ms\n", di.passes, di.total_ms);
            render.save_denoised_buffer(denoise.c_str());
            std::printf("%s\n", denoise.c_str());
        }
        if (!temporal_out.empty()) {
            if (temporal_denoise) {
                render.run_denoise_temporal(tdn);
                std::printf("temporal denoise: %u passes, device %.3f ms\n", render.last_denoise_info().passes, render.last_denoise_info().total_ms);
                render.save_denoised_buffer(temporal_out.c_str());
            } else render.save_temporal_buffer(temporal_out.c_str());
            std::printf("%s\n", temporal_out.c_str());
        }
        if (upsample) { // (last: it leaves the low frame's sums on the handle and its own AOV buffers)
            render.run_view_upsampled(task.eye_pos, inv_view, fov_y, upsample, up, upsample_guide_spp);
            const crt_upsample_info& ui = render.last_upsample_info();
            std::printf("upsample: factor %u, radius %u, %llu fallback pixels, device %.3f ms\n", upsample, up.radius, (unsigned long long)ui.fallback_pixels, ui.total_ms);
            render.save_upsampled_buffer(upsample_out.c_str());
            std::printf("%s\n", upsample_out.c_str());
        }
        render.free();
        return 0;
    } catch (const crt::Error& e) {
        std::fprintf(stderr, "crt_cli: %s (%s)\n", e.what(), crt_strerror(e.status));
        return 1;
    }
}
