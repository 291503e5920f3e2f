// Stand-alone C++ host on top of the C ABI (include/mcrt.h): the same sequence a patched
// Camera::sampleImage() runs, but the flattened scene comes from a scene image
// (*.mcrt) written by the flattener inside the reference host.
//
//   mcrt_render scene.mcrt out.f64 [--width W --height H --sqrtspp S] [--seed N] [--photon] [--device D | --devices D0,D1,...]
//               [--tga out.tga [--tonemapper hable|aces] [--exposure EV] [--gain EV] [--plain]] [--aov PREFIX]
//               [--denoise OUT.f64 [--denoise-iterations N]] [--denoise-variance OUT.f64 [--denoise-variance-out VAR.f64]]
//               [--denoise-dual OUT.f64 [--denoise-dual-out VAR.f64]] [--stats PREFIX] [--robust PREFIX [--robust-kappa X] [--robust-radius R]]
//               [--converge TARGET [--max-spp N]] [--exr OUT.exr [--exr-compression none|zip]]
//               [--adaptive TARGET [--max-spp N] [--adaptive-window R] [--adaptive-floor F] [--adaptive-count OUT.u32]]
//               [--matte PREFIX [--matte-key material|surface] [--matte-ranks N]] [--compare REF [--compare-layer PREFIX]]
//               [--occlusion PREFIX [--occlusion-rays N] [--occlusion-distance D]] [--lighting PREFIX]
//               [--light-groups PREFIX [--light-groups-by material|light|one] [--light-groups-depth D]]
//               [--path-classes PREFIX [--path-classes-depth D]]
//               [--film box|mitchell|catmull-rom|b-spline|hermite|gaussian|lanczos[,RADIUS[,CACHE]]]
//   mcrt_render scene.mcrt out.exr --probes POINTS.txt [--probe-order L] [--probe-rays N] [--seed N] [--device D]
//               [--light-groups-by material|light|one] [--light-groups-depth D] [--exr-compression none|zip]
//
// Writes the frame as raw FP64 RGB, row-major (what Image::operator() holds, camera/image.cpp:53-56),
// and prints the statistics. --tga also develops it the way Image::save does (auto exposure / gain, tone map, sRGB bytes:
// mcrt_tonemap) and writes the reference's .tga; the "image" options default to the ones stored in the scene image.
// --aov also writes the first-hit AOV frame of the same camera and seed (mcrt_render_aov, device 0): PREFIX.depth.f64, .position.f64,
// .normal.f64, .shading_normal.f64, .albedo.f64, .coverage.f64 (raw FP64, row-major) and PREFIX.surface.u32, .material.u32.
// --denoise also writes the frame filtered by mcrt_denoise (the edge-avoiding a-trous filter guided by that AOV frame; default parameters,
// --denoise-iterations N sets the one that sizes the footprint) as raw FP64 RGB, and with --tga develops the filtered frame too, to OUT's
// stem + ".tga".
// --denoise-variance renders the frame through mcrt_render_pixel_stats (the same frame) and also writes the frame filtered by
// mcrt_denoise_variance (the a-trous filter steered by the per-pixel sample variance; default parameters, --denoise-iterations N as above)
// as raw FP64 RGB - with --tga developed too, to OUT's stem + ".tga" -, and with --denoise-variance-out (refused without
// --denoise-variance) the filtered frame's variance, in the form mcrt_frame_noise reads; prints that summary for the unfiltered and the filtered frame (one device).
// --denoise-dual renders the frame through mcrt_render_pixel_stats (the same frame) and also writes the frame filtered by mcrt_denoise_dual
// (the dual-buffer non-local-means filter on the render's half-buffers; default parameters, no AOV pass) as raw FP64 RGB - with --tga
// developed too, to OUT's stem + ".tga" -, and with --denoise-dual-out (refused without --denoise-dual) the filtered frame's error
// estimate, in the form mcrt_frame_noise reads; prints that summary for the unfiltered and the filtered frame (one device).
// --stats renders the frame through mcrt_render_pixel_stats (the same frame) and also writes the per-pixel sample statistics,
// PREFIX.variance.f64, .half_a.f64 and .half_b.f64 (raw FP64 RGB, row-major), and prints the frame summary of mcrt_frame_noise (one device).
// --robust renders the frame through mcrt_render_highlights (the same frame; with --stats the statistics come from the same render) and
// also writes the robust frame of mcrt_robust_resolve, PREFIX.robust.f64 and PREFIX.removed.f64 (raw FP64 RGB) and PREFIX.clamped.u32,
// and prints how many pixels and samples were clamped and the luminance removed next to the frame's (one device).
// --converge renders the frame through mcrt_render_converged: batches of sqrtspp^2 samples at the seeds N, N + 1, ... merged until the
// frame's relative error (mcrt_frame_noise) is at most TARGET or one more batch would exceed --max-spp (default 1024); --stats, --robust,
// --denoise-variance and --denoise-dual then read the accumulated buffers at the accumulated sample count. Prints batches, spp and the final relative
// error (one device).
// --adaptive renders the frame through mcrt_render_adaptive (path tracer): the per-pixel stopping rule - batch 0 over the frame, every later
// batch over the list of the pixels whose own relative error is above TARGET (or that have such a pixel within --adaptive-window R pixels:
// 1 .. 4, 0 = the pixel alone; the default 1), with --adaptive-floor F the radiance below which a pixel's signal counts as F (the default is
// derived from the frame), until the list is empty or --max-spp (default 1024) is reached per pixel; --stats then writes the accumulated
// statistics, --adaptive-count the samples every pixel received ([H][W] uint32), and with --exr the count map goes into the file as the
// UINT channel samples.count. Prints batches, the number of samples, the smallest and largest count and the list's length per batch. Not
// with --converge, --robust, --denoise-variance or --denoise-dual, which read a uniform sample count (one device).
// --exr also writes everything the run produced - the frame and the buffers of --aov, --stats, --robust and the --denoise options - into
// one OpenEXR file (mcrt_exr_save) as named channels: R, G, B; depth.Z, position.X/Y/Z, normal.X/Y/Z, shading_normal.X/Y/Z, albedo.R/G/B,
// coverage.A, surface.id, material.id; variance.R/G/B, half_a.*, half_b.*; tops0.R .. tops3.B, level.Y; robust.*, removed.*, clamped.count;
// denoise.*, denoise_variance.*, denoise_variance.variance.*, denoise_dual.*, denoise_dual.variance.*. Colour is HALF; depth, position,
// variances and level FLOAT; ids and counts UINT. The attributes mcrt:spp, mcrt:seed, mcrt:integrator and mcrt:kernel say what was
// rendered. --exr-compression: zip (the default) or none. The .f64 outputs stay as they are (one device).
// --matte also writes the ranked id / coverage mattes of the same camera and seed (mcrt_render_matte, device 0; --matte-key material, the
// default, or surface; --matte-ranks N, default 6): PREFIX.id.u32 and PREFIX.coverage.f64 ([H][W][ranks]) and PREFIX.distinct.u32. With --exr
// the file also holds them as the Cryptomatte layer CryptoMaterial or CryptoSurface - FLOAT channels CryptoMaterial00.R/G/B/A, 01.*, ... -
// with the attributes cryptomatte/<key>/name, /hash, /conversion and /manifest (mcrt_matte_manifest); a manifest past 1 MiB (the surface
// key on large meshes) is left out, with a message: the ids then still separate the surfaces, without names.
// --compare compares the delivered frame with the reference frame REF (mcrt_frame_compare; default parameters, no mask) and prints one
// JSON line of the result; with --robust, --denoise, --denoise-variance or --denoise-dual each of those frames is compared too, a line
// each ("frame" names it). REF is raw little-endian binary64 of exactly width * height * 3 * 8 bytes, or a .npy file - version 1.0, '<f8',
// C order, shape (height, width, 3): what bench.py --dump-outputs writes - or a file that starts with the OpenEXR magic number (what --exr
// writes, or another renderer's scan-line file: mcrt_exr_open, mcrt_exr_load on device 0), of which the channels R, G, B - with
// --compare-layer PREFIX the channels PREFIX.R, PREFIX.G, PREFIX.B - are the reference; its data window must be width x height. With --exr
// the file also holds the error maps of the delivered frame as FLOAT channels error.se, error.rel and error.ssim (device 0).
// --occlusion also writes the occlusion pass of the same camera and seed (mcrt_render_occlusion, device 0; --occlusion-rays N rays per
// camera sample that hits, default 1, 64 at most; --occlusion-distance D: hits farther away do not occlude, default 0 = unbounded):
// PREFIX.ao.f64, PREFIX.sky.f64 ([H][W]) and PREFIX.bent_normal.f64 ([H][W][3], not normalised), raw FP64. With --exr the file also holds
// them as the HALF channels occlusion.ao, occlusion.sky and occlusion.bent.X/Y/Z.
// --lighting also writes the lighting passes of the same camera and seed (mcrt_render_lighting, device 0; path tracer only): PREFIX.emission.f64,
// .sky.f64, .direct.f64, .light.f64 and .unoccluded.f64 ([H][W][3], raw FP64). With --exr the file also holds them as the HALF channels
// lighting.emission.R/G/B ... lighting.unoccluded.R/G/B.
// --light-groups also writes the light groups of the same camera and seed (mcrt_render_light_groups, device 0; path tracer only): one plane
// per group of emitters and one for the sky, PREFIX.<name>.f64 ([height][width][3] FP64) and, with --exr, lightgroup.<name>.R/G/B (HALF).
// --light-groups-by material (default): a group per emissive material, named material<index>; light: a group per emitter surface,
// light<index>; one: every emitter in one group, lights. --light-groups-depth D cuts the paths (1 = direct light only; default 0 = whole).
// --path-classes also writes the path classes of the same camera and seed (mcrt_render_path_classes, device 0; path tracer only): the frame
// split by what the first surface did with the light, eight planes - emission, background, diffuse_direct, diffuse_indirect, glossy_direct,
// glossy_indirect, transmission_direct, transmission_indirect - as PREFIX.<name>.f64 ([height][width][3] FP64) and, with --exr,
// pathclass.<name>.R/G/B (HALF; the file then carries OpenEXR's long-names bit: pathclass.transmission_indirect.R is 33 bytes).
// --path-classes-depth D cuts the paths (1 = no indirect light; default 0 = whole).
// --lens orthographic|equirectangular|fisheye renders under a camera model (mcrt_set_lens, include/mcrt.h "Camera models"): the
// frame is then the light groups with every emitter and the sky in one plane (what the binding's Context.render_lens returns; path tracer,
// one device), and --aov, --matte, --occlusion, --lighting, --light-groups and --path-classes trace that lens's rays, their flags
// unchanged. --lens-fov DEG[,DEG]: fov_x and fov_y in degrees (equirectangular: default 360,180; fisheye: the full angle, default 180).
// --lens-width W: the orthographic frame's width in world units. Not with --photon, --adaptive, --converge, --stats, --robust,
// --denoise-variance, --denoise-dual or --devices: those make their camera rays inside a render kernel.
// --gather turns the run into a surface gather (mcrt_set_ray_source, include/mcrt.h "Ray sources"): the first-hit AOV pass of the camera
// is rendered first, its `position` and `normal` frames (--gather-normal shading: `shading_normal`) become a SURFACE ray source, and
// the frame - the light groups with everything in one plane, as under --lens - and --matte, --occlusion, --lighting, --light-groups
// and --path-classes then trace cosine-weighted rays from those surface points: the frame times pi is the irradiance that arrives at
// what each pixel sees, --light-groups gives it per lamp. --aov still writes the camera's own AOV frame. Not with --lens, nor with
// what --lens excludes.
// --probes turns the run into a light-probe bake (mcrt_render_probes, include/mcrt.h "Light probes"): POINTS.txt holds one point "x y z"
// per line (blank lines and lines that start with # are skipped), N points in all; from each --probe-rays rays (default 1024, rounded up
// to a square) leave uniformly over the sphere, and the light that travels along them is projected on the first (L + 1)^2 spherical
// harmonics (--probe-order L = 0, 1, 2; default 2), per light group (--light-groups-by, --light-groups-depth as above). The output - the
// second argument - is an N x 1 OpenEXR file (mcrt_exr_save) with the FLOAT channels probe.<plane>.<k>.R/G/B, the raw means (the header's
// constants normalise them); no frame is rendered. Path tracer on one device; not with --lens, --gather or any other output.
// --film NAME[,RADIUS[,CACHE]] sets the camera's reconstruction filter for the run (film_filter, film_radius - 0 or none: the filter's
// default -, film_cache_size - 0 or none: no table): the frame is then the filtered one, and --light-groups and --path-classes carry
// their FILM flag (include/mcrt.h "Filtered planes"): unclamped planes through the same filter, which add up to the frame; under
// --lens the frame itself is the light groups' single plane with FILM | CLAMP. Not with --gather (a ray
// source has no film positions).
// --devices renders the frame on several GPUs from this one process (mcrt_render_multi: one host thread per GPU).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/mcrt.h"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s scene.mcrt out.f64 [--width W --height H --sqrtspp S] [--seed N] [--photon] [--device D]\n", argv[0]);
        return 2;
    }
    mcrt_image* img = nullptr;
    if (mcrt_image_load(argv[1], &img) != MCRT_OK) {
        std::fprintf(stderr, "cannot load scene image %s\n", argv[1]);
        return 1;
    }
    mcrt_camera_desc cam = *mcrt_image_camera(img);
    uint32_t seed = (uint32_t)mcrt_image_param(img, "global_seed");
    int photon = (int)mcrt_image_param(img, "photon_mapping"), device = 0;
    auto from_bits = [](uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; };
    mcrt_image_desc image{};
    image.tonemapper = (uint32_t)mcrt_image_param(img, "image_tonemapper");
    image.plain = (uint32_t)mcrt_image_param(img, "image_plain");
    image.exposure_compensation = from_bits(mcrt_image_param(img, "image_exposure_ev_bits"));
    image.gain_compensation = from_bits(mcrt_image_param(img, "image_gain_ev_bits"));
    std::string tga, aov, denoise, dvar, dvar_out, ddual, ddual_out, pstats, robust, exr, matte, compare, compare_layer, occlusion, lighting, light_groups, light_groups_by = "material", path_classes;
    uint32_t light_groups_depth = 0, path_classes_depth = 0;
    std::string lens_name, film;
    mcrt_lens_desc lens{};
    std::string probes;
    uint32_t probe_order = MCRT_PROBE_ORDER_MAX, probe_rays = 1024;
    bool gather = false;
    std::string gather_normal = "normal";
    std::vector<double> gather_position, gather_normals;
    mcrt_occlusion_params oparams{};
    bool compare_exr = false;
    mcrt_matte_params mparams{};
    std::deque<std::string> exr_attr_text;  // the attributes --matte adds to --exr's: name, value, name, value, ...
    mcrt_exr_params eparams{};
    // what --exr writes: the channels, their names and the buffers that outlive the block that filled them
    std::vector<mcrt_exr_channel> exr_channels;
    std::deque<std::string> exr_names;
    std::deque<std::vector<double>> exr_f64;
    std::deque<std::vector<uint32_t>> exr_u32;
    auto exr_one = [&](const std::string& name, const void* data, uint32_t pixel_type, uint32_t stride, uint32_t offset) {
        if (exr.empty()) return;
        exr_names.push_back(name);
        exr_channels.push_back({exr_names.back().c_str(), data, pixel_type == MCRT_EXR_UINT ? (uint32_t)MCRT_EXR_SRC_U32 : (uint32_t)MCRT_EXR_SRC_F64, pixel_type, stride, offset});
    };
    auto exr_layer = [&](const std::string& layer, const char* parts, const void* data, uint32_t pixel_type, uint32_t stride = 3, uint32_t first = 0) {
        for (uint32_t i = 0; parts[i]; i++) exr_one(layer.empty() ? std::string(1, parts[i]) : layer + "." + parts[i], data, pixel_type, stride, first + i);
    };
    auto exr_keep = [&](std::vector<double>& v) { exr_f64.push_back(std::move(v)); return exr_f64.back().data(); };
    auto exr_keep_u32 = [&](std::vector<uint32_t>& v) { exr_u32.push_back(std::move(v)); return exr_u32.back().data(); };
    mcrt_robust_params rparams{};
    mcrt_denoise_params dparams{};
    mcrt_converge_params cparams{};
    bool converge = false, adaptive = false;
    mcrt_adaptive_params aparams{};
    std::string adaptive_count;
    std::vector<uint32_t> sample_count;
    std::vector<int> devices;
    for (int i = 3; i < argc; i++) {
        std::string k = argv[i];
        auto val = [&]() { return i + 1 < argc ? std::strtoul(argv[++i], nullptr, 0) : 0ul; };
        if (k == "--width") cam.width = (uint32_t)val();
        else if (k == "--height") cam.height = (uint32_t)val();
        else if (k == "--sqrtspp") cam.sqrtspp = (uint32_t)val();
        else if (k == "--seed") seed = (uint32_t)val();
        else if (k == "--device") device = (int)val();
        else if (k == "--devices" && i + 1 < argc) {
            for (const char* p = argv[++i]; *p;) {
                devices.push_back((int)std::strtol(p, const_cast<char**>(&p), 10));
                if (*p == ',') p++;
            }
        }
        else if (k == "--photon") photon = 1;
        else if (k == "--tga" && i + 1 < argc) tga = argv[++i];
        else if (k == "--aov" && i + 1 < argc) aov = argv[++i];
        else if (k == "--denoise" && i + 1 < argc) denoise = argv[++i];
        else if (k == "--denoise-variance" && i + 1 < argc) dvar = argv[++i];
        else if (k == "--denoise-variance-out" && i + 1 < argc) dvar_out = argv[++i];
        else if (k == "--denoise-dual" && i + 1 < argc) ddual = argv[++i];
        else if (k == "--denoise-dual-out" && i + 1 < argc) ddual_out = argv[++i];
        else if (k == "--stats" && i + 1 < argc) pstats = argv[++i];
        else if (k == "--robust" && i + 1 < argc) robust = argv[++i];
        else if (k == "--exr" && i + 1 < argc) exr = argv[++i];
        else if (k == "--matte" && i + 1 < argc) matte = argv[++i];
        else if (k == "--compare" && i + 1 < argc) compare = argv[++i];
        else if (k == "--occlusion" && i + 1 < argc) occlusion = argv[++i];
        else if (k == "--lighting" && i + 1 < argc) lighting = argv[++i];
        else if (k == "--light-groups" && i + 1 < argc) light_groups = argv[++i];
        else if (k == "--light-groups-by" && i + 1 < argc) light_groups_by = argv[++i];
        else if (k == "--light-groups-depth" && i + 1 < argc) light_groups_depth = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
        else if (k == "--path-classes" && i + 1 < argc) path_classes = argv[++i];
        else if (k == "--probes" && i + 1 < argc) probes = argv[++i];
        else if (k == "--probe-order") probe_order = (uint32_t)val();
        else if (k == "--probe-rays") probe_rays = (uint32_t)val();
        else if (k == "--gather") gather = true;
        else if (k == "--gather-normal" && i + 1 < argc) gather_normal = argv[++i];
        else if (k == "--lens" && i + 1 < argc) lens_name = argv[++i];
        else if (k == "--film" && i + 1 < argc) film = argv[++i];
        else if (k == "--lens-fov" && i + 1 < argc) {
            char* rest = nullptr;
            const double to_radians = 3.14159265358979323846 / 180.0;
            lens.fov_x = std::strtod(argv[++i], &rest) * to_radians;
            if (rest && *rest == ',') lens.fov_y = std::strtod(rest + 1, nullptr) * to_radians;
        } else if (k == "--lens-width" && i + 1 < argc) lens.width_world = std::strtod(argv[++i], nullptr);
        else if (k == "--path-classes-depth" && i + 1 < argc) path_classes_depth = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
        else if (k == "--occlusion-rays") oparams.rays = (uint32_t)val();
        else if (k == "--occlusion-distance" && i + 1 < argc) oparams.max_distance = std::strtod(argv[++i], nullptr);
        else if (k == "--compare-layer" && i + 1 < argc) compare_layer = argv[++i];
        else if (k == "--matte-key" && i + 1 < argc) mparams.key = (argv[++i][0] | 0x20) == 's' ? MCRT_MATTE_SURFACE : MCRT_MATTE_MATERIAL;
        else if (k == "--matte-ranks") mparams.ranks = (uint32_t)val();
        else if (k == "--exr-compression" && i + 1 < argc) eparams.compression = MCRT_EXR_COMPRESSION_SET | ((argv[++i][0] | 0x20) == 'n' ? MCRT_EXR_COMPRESSION_NONE : MCRT_EXR_COMPRESSION_ZIP);
        else if (k == "--robust-kappa" && i + 1 < argc) rparams.kappa = std::strtod(argv[++i], nullptr);
        else if (k == "--robust-radius") rparams.radius = (uint32_t)val();
        else if (k == "--converge" && i + 1 < argc) converge = true, cparams.target_relative_error = std::strtod(argv[++i], nullptr);
        else if (k == "--max-spp") cparams.max_spp = aparams.max_spp = (uint32_t)val();
        else if (k == "--adaptive" && i + 1 < argc) adaptive = true, aparams.target_relative_error = std::strtod(argv[++i], nullptr);
        else if (k == "--adaptive-window") {
            const uint32_t r = (uint32_t)val();
            aparams.window = r == 0 ? MCRT_ADAPTIVE_WINDOW_NONE : r;
        } else if (k == "--adaptive-floor" && i + 1 < argc) aparams.floor = std::strtod(argv[++i], nullptr);
        else if (k == "--adaptive-count" && i + 1 < argc) adaptive_count = argv[++i];
        else if (k == "--denoise-iterations") dparams.iterations = (uint32_t)val();
        else if (k == "--tonemapper" && i + 1 < argc) image.tonemapper = (argv[++i][0] | 0x20) == 'a' ? MCRT_TONEMAP_ACES : MCRT_TONEMAP_HABLE;
        else if (k == "--exposure" && i + 1 < argc) image.exposure_compensation = std::strtod(argv[++i], nullptr);
        else if (k == "--gain" && i + 1 < argc) image.gain_compensation = std::strtod(argv[++i], nullptr);
        else if (k == "--plain") image.plain = 1;
    }
    if (!dvar_out.empty() && dvar.empty()) {
        std::fprintf(stderr, "--denoise-variance-out needs --denoise-variance\n");
        return 2;
    }
    if (!ddual_out.empty() && ddual.empty()) {
        std::fprintf(stderr, "--denoise-dual-out needs --denoise-dual\n");
        return 2;
    }
    cam.shard_index = 0;
    cam.shard_count = 1;
    if (!film.empty()) {  // NAME[,RADIUS[,CACHE]]
        const char* const filters[] = {"box", "mitchell", "catmull-rom", "b-spline", "hermite", "gaussian", "lanczos"};
        const std::string name = film.substr(0, film.find(','));
        uint32_t filter = 0;
        while (filter < 7 && name != filters[filter]) filter++;
        if (filter == 7) {
            std::fprintf(stderr, "--film: box, mitchell, catmull-rom, b-spline, hermite, gaussian or lanczos, not %s\n", name.c_str());
            return 2;
        }
        if (gather) {
            std::fprintf(stderr, "--film is not for --gather: a ray source's pixels have no film position\n");
            return 2;
        }
        cam.film_filter = filter;
        cam.film_radius = 0.0;
        cam.film_cache_size = 0;
        if (name.size() < film.size()) {
            char* rest = nullptr;
            cam.film_radius = std::strtod(film.c_str() + name.size() + 1, &rest);
            if (rest && *rest == ',') cam.film_cache_size = (uint32_t)std::strtoul(rest + 1, nullptr, 10);
        }
    }
    // --compare's reference, read before anything is rendered: raw binary64, or .npy 1.0 of '<f8' in C order and shape (height, width, 3)
    std::vector<double> reference;
    if (!compare.empty()) {
        const size_t want = (size_t)cam.width * cam.height * 3 * 8;
        std::string bytes;
        if (FILE* in = std::fopen(compare.c_str(), "rb")) {
            char chunk[1 << 16];
            for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, in)) > 0;) bytes.append(chunk, got);
            std::fclose(in);
        } else {
            std::fprintf(stderr, "--compare: cannot read %s\n", compare.c_str());
            return 1;
        }
        size_t at = 0;
        compare_exr = bytes.size() >= 4 && bytes.compare(0, 4, "\x76\x2f\x31\x01") == 0;  // (read once a context is there)
        if (bytes.size() >= 10 && bytes.compare(0, 6, "\x93NUMPY") == 0) {
            const size_t len = (unsigned char)bytes[8] | (size_t)(unsigned char)bytes[9] << 8;
            const std::string head = bytes.size() >= 10 + len ? bytes.substr(10, len) : std::string();
            std::string h;  // the header's dict without blanks and quotes
            for (char c : head)
                if (c != ' ' && c != '"' && c != '\'') h += c;
            const std::string shape = "shape:(" + std::to_string(cam.height) + "," + std::to_string(cam.width) + ",3)";
            if (bytes[6] != 1 || bytes[7] != 0 || h.find("descr:<f8") == std::string::npos || h.find("fortran_order:False") == std::string::npos ||
                h.find(shape) == std::string::npos) {
                std::fprintf(stderr, "--compare: %s is not .npy 1.0 of '<f8' in C order with %s: %s\n", compare.c_str(), shape.c_str(), head.c_str());
                return 2;
            }
            at = 10 + len;
        }
        if (!compare_exr && bytes.size() - at != want) {
            std::fprintf(stderr, "--compare: %s holds %zu bytes of frame, %u x %u x 3 binary64 are %zu\n", compare.c_str(), bytes.size() - at, cam.width, cam.height, want);
            return 2;
        }
        reference.resize(want / 8);
        if (!compare_exr) std::memcpy(reference.data(), bytes.data() + at, want);
    }
    // the groups of --light-groups-by: surface_group and the planes' names without the sky's (false: a message was printed)
    auto light_group_map = [&](std::vector<uint32_t>& group, std::vector<std::string>& names) {
        // the groups of light_group_map (the Python binding): emitters are the surfaces whose material carries MCRT_MAT_EMISSIVE
        const mcrt_scene_desc* sd = mcrt_image_scene(img);
        group.assign(sd->num_surfaces, 0u);
        names.clear();
        if (light_groups_by == "material") {
            std::vector<int> group_of(sd->num_materials, -1);
            for (uint32_t m = 0; m < sd->num_materials; m++) {
                if (!(sd->materials[m].flags & MCRT_MAT_EMISSIVE)) continue;
                bool used = false;
                for (uint32_t i = 0; i < sd->num_surfaces && !used; i++) used = sd->surf_material[i] == m;
                if (!used) continue;
                group_of[m] = (int)names.size();
                names.push_back("material" + std::to_string(m));
            }
            for (uint32_t i = 0; i < sd->num_surfaces; i++)
                if (group_of[sd->surf_material[i]] >= 0) group[i] = (uint32_t)group_of[sd->surf_material[i]];
        } else if (light_groups_by == "light") {
            for (uint32_t i = 0; i < sd->num_surfaces; i++)
                if (sd->materials[sd->surf_material[i]].flags & MCRT_MAT_EMISSIVE) {
                    group[i] = (uint32_t)names.size();
                    names.push_back("light" + std::to_string(i));
                }
        } else if (light_groups_by != "one") {
            std::fprintf(stderr, "--light-groups-by: material, light or one, not %s\n", light_groups_by.c_str());
            return false;
        }
        if (names.empty()) names.push_back("lights");
        if (names.size() > MCRT_LIGHT_GROUPS_MAX) {
            std::fprintf(stderr, "--light-groups-by %s: %zu groups, at most %u can be rendered\n", light_groups_by.c_str(), names.size(), MCRT_LIGHT_GROUPS_MAX);
            return false;
        }
        return true;
    };
    if (!probes.empty() && (!lens_name.empty() || gather || photon || adaptive || converge || devices.size() > 1 || !exr.empty() || !tga.empty() || !aov.empty() || !denoise.empty() ||
                            !dvar.empty() || !ddual.empty() || !pstats.empty() || !robust.empty() || !matte.empty() || !compare.empty() || !occlusion.empty() ||
                            !lighting.empty() || !light_groups.empty() || !path_classes.empty())) {
        std::fprintf(stderr, "--probes is a run of its own on one device: the path tracer's probes into the OpenEXR file named as the output, with --probe-order, --probe-rays, "
                             "--light-groups-by, --light-groups-depth, --seed, --device and --exr-compression only\n");
        return 2;
    }
    if (!probes.empty() && (probe_order > MCRT_PROBE_ORDER_MAX || probe_rays == 0)) {
        std::fprintf(stderr, "--probe-order: 0, 1 or 2; --probe-rays: at least 1\n");
        return 2;
    }
    if (!lens_name.empty()) {
        const char* models[] = {"orthographic", "equirectangular", "fisheye"};
        for (uint32_t m = 0; m < 3; m++)
            if (lens_name == models[m]) lens.model = MCRT_LENS_ORTHOGRAPHIC + m;
        if (lens.model == MCRT_LENS_NONE) {
            std::fprintf(stderr, "--lens: orthographic, equirectangular or fisheye, not %s\n", lens_name.c_str());
            return 2;
        }
        if (photon || adaptive || converge || !pstats.empty() || !robust.empty() || !dvar.empty() || !ddual.empty() || devices.size() > 1) {
            std::fprintf(stderr, "--lens is the path tracer on one device (not with --photon or --devices), and not with --adaptive, --converge, --stats, --robust, --denoise-variance or --denoise-dual\n");
            return 2;
        }
    }
    if (gather) {
        if (gather_normal != "normal" && gather_normal != "shading") {
            std::fprintf(stderr, "--gather-normal: normal or shading, not %s\n", gather_normal.c_str());
            return 2;
        }
        if (!lens_name.empty() || photon || adaptive || converge || !pstats.empty() || !robust.empty() || !dvar.empty() || !ddual.empty() || devices.size() > 1) {
            std::fprintf(stderr, "--gather is the path tracer on one device (not with --photon or --devices), and not with --lens, --adaptive, --converge, --stats, --robust, --denoise-variance or --denoise-dual\n");
            return 2;
        }
    } else if (gather_normal != "normal") {
        std::fprintf(stderr, "--gather-normal needs --gather\n");
        return 2;
    }
    if (lens_name.empty() && (lens.fov_x != 0.0 || lens.fov_y != 0.0 || lens.width_world != 0.0)) {
        std::fprintf(stderr, "--lens-fov and --lens-width need --lens\n");
        return 2;
    }
    if (devices.empty()) devices.push_back(device);
    if (!exr.empty() && devices.size() > 1) {
        std::fprintf(stderr, "--exr takes one device\n");
        return 2;
    }
    std::vector<mcrt_ctx*> ctxs(devices.size(), nullptr);
    int rc = MCRT_OK;
    for (size_t d = 0; d < devices.size() && rc == MCRT_OK; d++) {
        if (mcrt_create(&ctxs[d], devices[d]) != MCRT_OK) {
            std::fprintf(stderr, "mcrt_create(device %d): %s\n", devices[d], mcrt_last_error(nullptr));
            return 1;
        }
        rc = mcrt_upload_scene(ctxs[d], mcrt_image_scene(img));
        if (rc == MCRT_OK && photon)
            rc = mcrt_upload_photons(ctxs[d], mcrt_image_photons(img, 0), mcrt_image_photons(img, 1),
                                     (uint32_t)mcrt_image_param(img, "k_nearest_photons"), (int)mcrt_image_param(img, "direct_visualization"));
        if (rc != MCRT_OK) std::fprintf(stderr, "device %d: %s\n", devices[d], mcrt_last_error(ctxs[d]));
    }
    mcrt_ctx* ctx = ctxs[0];
    if (!probes.empty()) {  // the probe bake: no frame
        if (rc != MCRT_OK) return 1;
        std::vector<double> points;
        if (FILE* in = std::fopen(probes.c_str(), "r")) {
            char line[512];
            while (std::fgets(line, sizeof line, in)) {
                const char* t = line + std::strspn(line, " \t\r\n");
                if (!*t || *t == '#') continue;
                double v[3];
                if (std::sscanf(t, "%lf %lf %lf", &v[0], &v[1], &v[2]) != 3) {
                    std::fclose(in);
                    std::fprintf(stderr, "--probes: %s: not a point \"x y z\": %s", probes.c_str(), line);
                    return 2;
                }
                points.insert(points.end(), v, v + 3);
            }
            std::fclose(in);
        } else {
            std::fprintf(stderr, "--probes: cannot read %s\n", probes.c_str());
            return 1;
        }
        if (points.empty()) {
            std::fprintf(stderr, "--probes: %s holds no point\n", probes.c_str());
            return 2;
        }
        std::vector<uint32_t> group;
        std::vector<std::string> names;
        if (!light_group_map(group, names)) return 1;
        mcrt_probe_params pp{};
        pp.groups.num_groups = (uint32_t)names.size();
        pp.groups.max_depth = light_groups_depth;
        pp.groups.surface_group = group.data();
        pp.order = probe_order;
        pp.positions = points.data();
        names.push_back("sky");
        mcrt_camera_desc pcam{};
        pcam.width = (uint32_t)(points.size() / 3);
        pcam.height = 1;
        pcam.shard_count = 1;
        for (pcam.sqrtspp = 1; (uint64_t)pcam.sqrtspp * pcam.sqrtspp < probe_rays;) pcam.sqrtspp++;
        const uint32_t K = mcrt_probe_coefficients(probe_order);
        const size_t frame = (size_t)pcam.width * 3;
        std::vector<double> coefficients(names.size() * K * frame);
        mcrt_stats pst;
        rc = mcrt_render_probes(ctx, &pcam, seed, &pp, coefficients.data(), &pst);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        exr = argv[2];
        for (size_t p = 0; p < names.size(); p++)
            for (uint32_t k = 0; k < K; k++) exr_layer("probe." + names[p] + "." + std::to_string(k), "RGB", coefficients.data() + (p * K + k) * frame, MCRT_EXR_FLOAT);
        const std::string a_rays = std::to_string(pcam.sqrtspp * pcam.sqrtspp), a_seed = std::to_string(seed), a_order = std::to_string(probe_order);
        const mcrt_exr_attribute attributes[] = {{"mcrt:probe_rays", a_rays.c_str()}, {"mcrt:seed", a_seed.c_str()}, {"mcrt:probe_order", a_order.c_str()}};
        mcrt_exr_result er;
        mcrt_stats est;
        rc = mcrt_exr_save(ctx, exr.c_str(), pcam.width, 1, exr_channels.data(), (uint32_t)exr_channels.size(), attributes, 3, &eparams, &er, &est);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        std::printf("{\"probes\":%u,\"rays\":%u,\"order\":%u,\"planes\":%zu,\"by\":\"%s\",\"max_depth\":%u,\"exr\":\"%s\",\"channels\":%zu,\"traced\":%llu,\"kernel_ms\":%.3f,\"total_ms\":%.3f}\n",
                    pcam.width, pcam.sqrtspp * pcam.sqrtspp, probe_order, names.size(), light_groups_by.c_str(), light_groups_depth, exr.c_str(), exr_channels.size(),
                    (unsigned long long)pst.rays, pst.kernel_ms, pst.total_ms);
        for (mcrt_ctx* c : ctxs) mcrt_destroy(c);
        mcrt_image_free(img);
        return 0;
    }
    auto set_gather = [&]() {  // (pixels with no hit hold a zero normal: the kernel's fallback, +z from the origin)
        mcrt_ray_source_desc d{};
        d.kind = MCRT_RAY_SOURCE_SURFACE;
        d.pixels = (uint64_t)cam.width * cam.height;
        d.first = gather_position.data();
        d.second = gather_normals.data();
        d.offset = 1e-9;
        uint64_t sanitised = 0;
        const int r = mcrt_set_ray_source_host(ctx, &d, &sanitised);
        if (r == MCRT_OK) std::printf("{\"gather\":\"%s\",\"pixels\":%llu,\"without_surface\":%llu}\n", gather_normal.c_str(), (unsigned long long)d.pixels, (unsigned long long)sanitised);
        return r;
    };
    if (rc == MCRT_OK && lens.model != MCRT_LENS_NONE) rc = mcrt_set_lens(ctx, &lens);
    if (compare_exr && rc == MCRT_OK) {  // the reference's channels, widened on the device into the [H][W][3] frame
        mcrt_exr_file* ref = nullptr;
        mcrt_exr_info info{};
        if (mcrt_exr_open(ctx, compare.c_str(), &ref) != MCRT_OK || mcrt_exr_file_info(ref, &info) != MCRT_OK) {
            std::fprintf(stderr, "--compare: %s\n", mcrt_last_error(ctx));
            return 1;
        }
        if (info.width != cam.width || info.height != cam.height) {
            std::fprintf(stderr, "--compare: %s is %u x %u, the frame %u x %u\n", compare.c_str(), info.width, info.height, cam.width, cam.height);
            mcrt_exr_close(ref);
            return 2;
        }
        std::string names[3];
        mcrt_exr_target targets[3];
        for (uint32_t c = 0; c < 3; c++) {
            names[c] = (compare_layer.empty() ? std::string() : compare_layer + ".") + "RGB"[c];
            targets[c] = mcrt_exr_target{names[c].c_str(), reference.data(), MCRT_EXR_SRC_F64, 3, c, 0};
        }
        const int lrc = mcrt_exr_load(ctx, ref, targets, 3, nullptr, nullptr, nullptr);
        mcrt_exr_close(ref);
        if (lrc != MCRT_OK) {
            std::fprintf(stderr, "--compare: %s\n", mcrt_last_error(ctx));
            return lrc == MCRT_ERR_INVALID ? 2 : 1;
        }
    }
    std::vector<double> rgb((size_t)cam.width * cam.height * 3);
    mcrt_stats st;
    const int mode = photon ? MCRT_INTEGRATOR_PHOTON_MAPPER : MCRT_INTEGRATOR_PATH_TRACER;
    std::vector<double> variance, half_a, half_b;
    std::vector<double> tops, level;
    uint32_t spp = cam.sqrtspp * cam.sqrtspp;  // of the delivered frame: --converge accumulates batches of that many
    if (adaptive && (converge || photon || !robust.empty() || !dvar.empty() || !ddual.empty() || ctxs.size() > 1)) {
        std::fprintf(stderr, "--adaptive is the path tracer on one device, and not with --converge, --robust, --denoise-variance or --denoise-dual\n");
        return 2;
    }
    if (rc == MCRT_OK && adaptive) {
        if (!pstats.empty()) {
            variance.resize(rgb.size());
            half_a.resize(rgb.size());
            half_b.resize(rgb.size());
        }
        const mcrt_pixel_stats_buffers b{pstats.empty() ? nullptr : variance.data(), pstats.empty() ? nullptr : half_a.data(), pstats.empty() ? nullptr : half_b.data()};
        sample_count.resize(rgb.size() / 3);
        mcrt_adaptive_result ar;
        rc = mcrt_render_adaptive(ctx, &cam, seed, &aparams, rgb.data(), &b, sample_count.data(), &ar, &st);
        if (rc == MCRT_OK) {
            spp = ar.max_count;
            std::string active;
            for (uint32_t j = 0; j < ar.batches && j < MCRT_CONVERGE_TRACE; j++) active += (j ? "," : "") + std::to_string(ar.active[j]);
            std::printf("{\"adaptive\":%.17g,\"batches\":%u,\"samples\":%llu,\"min_count\":%u,\"max_count\":%u,\"active\":[%s]}\n", aparams.target_relative_error,
                        ar.batches, (unsigned long long)ar.samples, ar.min_count, ar.max_count, active.c_str());
            if (!adaptive_count.empty()) {
                FILE* fc = std::fopen(adaptive_count.c_str(), "wb");
                if (!fc || std::fwrite(sample_count.data(), 4, sample_count.size(), fc) != sample_count.size()) {
                    std::fprintf(stderr, "cannot write %s\n", adaptive_count.c_str());
                    return 1;
                }
                std::fclose(fc);
            }
        }
    } else if (rc == MCRT_OK && (converge || !pstats.empty() || !robust.empty() || !dvar.empty() || !ddual.empty())) {
        if (ctxs.size() > 1) {
            std::fprintf(stderr, "--stats, --robust, --denoise-variance, --denoise-dual and --converge take one device\n");
            return 2;
        }
        if (!dvar.empty()) variance.resize(rgb.size());
        const bool ps = !pstats.empty() || !ddual.empty();  // the three statistics
        if (ps) {
            variance.resize(rgb.size());
            half_a.resize(rgb.size());
            half_b.resize(rgb.size());
        }
        const mcrt_pixel_stats_buffers b{ps || !dvar.empty() ? variance.data() : nullptr, ps ? half_a.data() : nullptr, ps ? half_b.data() : nullptr};
        if (!robust.empty()) {
            tops.resize(rgb.size() * MCRT_ROBUST_TOPS);
            level.resize(rgb.size() / 3);
        }
        const mcrt_highlight_buffers h{robust.empty() ? nullptr : tops.data(), robust.empty() ? nullptr : level.data()};
        if (converge) {
            mcrt_converge_result cr;
            rc = mcrt_render_converged(ctx, &cam, seed, mode, &cparams, rgb.data(), &b, &h, &cr, &st);
            if (rc == MCRT_OK) {
                spp = cr.spp;
                std::printf("{\"converge\":%.17g,\"batches\":%u,\"spp\":%u,\"relative_error\":%.17g,\"noise\":%.17g,\"signal\":%.17g}\n",
                            cparams.target_relative_error, cr.batches, cr.spp, cr.final.relative_error, cr.final.noise, cr.final.signal);
            }
        } else if (!robust.empty())
            rc = mcrt_render_highlights(ctx, &cam, seed, mode, rgb.data(), &h, &b, &st);
        else
            rc = mcrt_render_pixel_stats(ctx, &cam, seed, mode, rgb.data(), &b, &st);
    } else if (rc == MCRT_OK && (lens.model != MCRT_LENS_NONE || gather)) {  // the frame under the lens or the source: everything in plane 0 of the light groups
        if (gather) {  // the camera's first hits become the surface points the rays start from
            const size_t px = (size_t)cam.width * cam.height;
            gather_position.assign(px * 3, 0.0);
            gather_normals.assign(px * 3, 0.0);
            mcrt_aov_buffers gb{};
            gb.position = gather_position.data();
            (gather_normal == "shading" ? gb.shading_normal : gb.normal) = gather_normals.data();
            rc = mcrt_render_aov(ctx, &cam, seed, &gb, nullptr);
            if (rc == MCRT_OK) rc = set_gather();
            if (rc != MCRT_OK) {
                std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
                return 1;
            }
        }
        mcrt_light_group_params one{};
        one.num_groups = 1;
        one.flags = MCRT_LIGHT_GROUPS_SKY_PLANE | (film.empty() ? 0u : MCRT_LIGHT_GROUPS_FILM | MCRT_LIGHT_GROUPS_FILM_CLAMP);
        one.sky_plane = 0;
        rc = mcrt_render_light_groups(ctx, &cam, seed, &one, rgb.data(), &st);
    } else if (rc == MCRT_OK)
        rc = ctxs.size() > 1 ? mcrt_render_multi(ctxs.data(), (uint32_t)ctxs.size(), &cam, seed, mode, rgb.data(), &st)
                             : mcrt_render(ctx, &cam, seed, mode, rgb.data(), &st);
    if (rc != MCRT_OK) {
        std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
        return 1;
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(rgb.data(), sizeof(double), rgb.size(), f) != rgb.size()) {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    std::fclose(f);
    exr_layer("", "RGB", rgb.data(), MCRT_EXR_HALF);
    if (!sample_count.empty()) exr_one("samples.count", sample_count.data(), MCRT_EXR_UINT, 1, 0);
    // --compare: one JSON line per frame; with_maps (the delivered frame under --exr): its error maps become channels
    auto compare_frame = [&](const char* label, const std::vector<double>& frame, bool with_maps) {
        if (compare.empty()) return true;
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<double> se(with_maps ? px : 0), rel(with_maps ? px : 0), ssim(with_maps ? px : 0);
        const mcrt_compare_maps maps{with_maps ? se.data() : nullptr, with_maps ? rel.data() : nullptr, with_maps ? ssim.data() : nullptr};
        mcrt_compare_result r;
        mcrt_stats cst;
        const int crc = mcrt_frame_compare(ctx, cam.width, cam.height, frame.data(), reference.data(), nullptr, nullptr, &maps, &r, &cst);
        if (crc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", crc, mcrt_last_error(ctx));
            return false;
        }
        char psnr[40];
        std::snprintf(psnr, sizeof psnr, r.mse == 0.0 && r.compared ? "\"inf\"" : "%.17g", r.psnr);
        std::printf("{\"compare\":\"%s\",\"frame\":\"%s\",\"mse\":%.17g,\"rmse\":%.17g,\"mae\":%.17g,\"relmse\":%.17g,\"psnr\":%s,\"mean_ssim\":%.17g,"
                    "\"max_abs\":%.17g,\"max_abs_pixel\":%lld,\"max_abs_channel\":%d,\"compared\":%llu,\"nonfinite\":%llu,\"differing\":%llu,"
                    "\"ssim_centres\":%llu,\"ssim_excluded\":%llu,\"sum_se\":%.17g,\"sum_ae\":%.17g,\"sum_rel\":%.17g,\"sum_ssim\":%.17g,\"kernel_ms\":%.3f,\"total_ms\":%.3f}\n",
                    compare.c_str(), label, r.mse, r.rmse, r.mae, r.relmse, psnr, r.mean_ssim, r.max_abs, r.compared ? (long long)r.max_abs_pixel : -1ll,
                    r.compared ? (int)r.max_abs_channel : -1, (unsigned long long)r.compared, (unsigned long long)r.nonfinite, (unsigned long long)r.differing,
                    (unsigned long long)r.ssim_centres, (unsigned long long)r.ssim_excluded, r.sum_se, r.sum_ae, r.sum_rel, r.sum_ssim, cst.kernel_ms, cst.total_ms);
        if (with_maps) {
            exr_one("error.se", exr_keep(se), MCRT_EXR_FLOAT, 1, 0);
            exr_one("error.rel", exr_keep(rel), MCRT_EXR_FLOAT, 1, 0);
            exr_one("error.ssim", exr_keep(ssim), MCRT_EXR_FLOAT, 1, 0);
        }
        return true;
    };
    if (!compare_frame("rgb", rgb, !exr.empty())) return 1;
    if (!variance.empty()) exr_layer("variance", "RGB", variance.data(), MCRT_EXR_FLOAT);
    if (!half_a.empty()) exr_layer("half_a", "RGB", half_a.data(), MCRT_EXR_HALF);
    if (!half_b.empty()) exr_layer("half_b", "RGB", half_b.data(), MCRT_EXR_HALF);
    if (!tops.empty()) {
        for (uint32_t k = 0; k < MCRT_ROBUST_TOPS; k++) exr_layer("tops" + std::to_string(k), "RGB", tops.data(), MCRT_EXR_HALF, 3 * MCRT_ROBUST_TOPS, 3 * k);
        exr_layer("level", "Y", level.data(), MCRT_EXR_FLOAT, 1);
    }
    if (!pstats.empty()) {
        const struct {
            const char* ext;
            const std::vector<double>* data;
        } files[3] = {{".variance.f64", &variance}, {".half_a.f64", &half_a}, {".half_b.f64", &half_b}};
        for (const auto& c : files) {
            const std::string path = pstats + c.ext;
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(c.data->data(), sizeof(double), c.data->size(), o) == c.data->size();
            if (o) std::fclose(o);
            if (!ok) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                return 1;
            }
        }
        mcrt_frame_noise_result fn{};
        if (!adaptive) rc = mcrt_frame_noise(ctx, (uint64_t)cam.width * cam.height, spp, rgb.data(), variance.data(), &fn);  // (one count for the frame)
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        if (!adaptive)
            std::printf("{\"stats\":\"%s\",\"noise\":%.17g,\"signal\":%.17g,\"relative_error\":%.17g,\"pixels\":%llu}\n", pstats.c_str(), fn.noise, fn.signal,
                    fn.relative_error, (unsigned long long)fn.pixels);
    }
    if (!robust.empty()) {
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<double> out(px * 3), removed(px * 3);
        std::vector<uint32_t> clamped(px);
        const mcrt_robust_buffers b{removed.data(), clamped.data()};
        mcrt_stats rst;
        rc = mcrt_robust_resolve(ctx, cam.width, cam.height, spp, rgb.data(), tops.data(), level.data(), &rparams, out.data(), &b, &rst);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        const struct {
            const char* ext;
            const void* data;
            size_t bytes;
        } files[3] = {{".robust.f64", out.data(), px * 24}, {".removed.f64", removed.data(), px * 24}, {".clamped.u32", clamped.data(), px * 4}};
        for (const auto& c : files) {
            const std::string path = robust + c.ext;
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(c.data, 1, c.bytes, o) == c.bytes;
            if (o) std::fclose(o);
            if (!ok) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                return 1;
            }
        }
        unsigned long long pixels = 0, samples = 0;
        double gone = 0.0, all = 0.0;  // luminance, added up in pixel order
        for (size_t p = 0; p < px; p++) {
            pixels += clamped[p] ? 1 : 0;
            samples += clamped[p];
            gone += (0.2126 * removed[p * 3] + 0.7152 * removed[p * 3 + 1]) + 0.0722 * removed[p * 3 + 2];
            all += (0.2126 * rgb[p * 3] + 0.7152 * rgb[p * 3 + 1]) + 0.0722 * rgb[p * 3 + 2];
        }
        std::printf("{\"robust\":\"%s\",\"clamped_pixels\":%llu,\"clamped_samples\":%llu,\"removed_energy\":%.17g,\"frame_energy\":%.17g,"
                    "\"removed_fraction\":%.17g,\"kernel_ms\":%.3f}\n",
                    robust.c_str(), pixels, samples, gone, all, all > 0.0 ? gone / all : 0.0, rst.kernel_ms);
        if (!compare_frame("robust", out, false)) return 1;
        if (!exr.empty()) {
            exr_layer("robust", "RGB", exr_keep(out), MCRT_EXR_HALF);
            exr_layer("removed", "RGB", exr_keep(removed), MCRT_EXR_HALF);
            exr_one("clamped.count", exr_keep_u32(clamped), MCRT_EXR_UINT, 1, 0);
        }
    }
    auto develop = [&](const std::vector<double>& frame, const std::string& path) {
        image.width = cam.width;
        image.height = cam.height;
        std::vector<uint8_t> bgr((size_t)cam.width * cam.height * 3);
        double factors[2];
        int r = mcrt_tonemap(ctx, frame.data(), &image, bgr.data(), factors);
        if (r == MCRT_OK) r = mcrt_tga_save(path.c_str(), cam.width, cam.height, bgr.data());
        if (r != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d writing %s: %s\n", r, path.c_str(), mcrt_last_error(ctx));
            return false;
        }
        std::printf("{\"tga\":\"%s\",\"exposure_factor\":%.17g,\"gain_factor\":%.17g}\n", path.c_str(), factors[0], factors[1]);
        return true;
    };
    if (!tga.empty() && !develop(rgb, tga)) return 1;
    if (!ddual.empty()) {
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<double> filtered(px * 3), filtered_var(px * 3);
        const mcrt_denoise_dual_buffers out{filtered.data(), filtered_var.data(), nullptr, nullptr};
        mcrt_stats dst;
        mcrt_frame_noise_result raw, fn;
        rc = mcrt_denoise_dual(ctx, cam.width, cam.height, spp, half_a.data(), half_b.data(), variance.data(), nullptr, &out, &dst);
        if (rc == MCRT_OK) rc = mcrt_frame_noise(ctx, px, spp, rgb.data(), variance.data(), &raw);
        if (rc == MCRT_OK) rc = mcrt_frame_noise(ctx, px, spp, filtered.data(), filtered_var.data(), &fn);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        const struct {
            const std::string* path;
            const std::vector<double>* data;
        } files[2] = {{&ddual, &filtered}, {&ddual_out, &filtered_var}};
        for (const auto& c : files) {
            if (c.path->empty()) continue;
            FILE* o = std::fopen(c.path->c_str(), "wb");
            const bool ok = o && std::fwrite(c.data->data(), sizeof(double), c.data->size(), o) == c.data->size();
            if (o) std::fclose(o);
            if (!ok) {
                std::fprintf(stderr, "cannot write %s\n", c.path->c_str());
                return 1;
            }
        }
        std::printf("{\"denoise_dual\":\"%s\",\"kernel_launches\":%u,\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"relative_error_raw\":%.17g,"
                    "\"relative_error\":%.17g}\n",
                    ddual.c_str(), dst.kernel_launches, dst.kernel_ms, dst.total_ms, raw.relative_error, fn.relative_error);
        if (!compare_frame("denoise_dual", filtered, false)) return 1;
        if (!tga.empty()) {
            const size_t dot = ddual.find_last_of('.'), slash = ddual.find_last_of('/');
            const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
            if (!develop(filtered, (has_ext ? ddual.substr(0, dot) : ddual) + ".tga")) return 1;
        }
        if (!exr.empty()) {
            exr_layer("denoise_dual", "RGB", exr_keep(filtered), MCRT_EXR_HALF);
            exr_layer("denoise_dual.variance", "RGB", exr_keep(filtered_var), MCRT_EXR_FLOAT);
        }
    }
    if (!aov.empty() || !denoise.empty() || !dvar.empty()) {
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<double> depth(px), position(px * 3), normal(px * 3), shading_normal(px * 3), albedo(px * 3), coverage(px);
        std::vector<uint32_t> surface(px), material(px);
        const mcrt_aov_buffers b{depth.data(), position.data(), normal.data(), shading_normal.data(), albedo.data(), coverage.data(), surface.data(), material.data()};
        mcrt_stats ast;
        if (gather) (void)mcrt_set_ray_source(ctx, nullptr);  // (the camera's own AOV frame)
        rc = mcrt_render_aov(ctx, &cam, seed, &b, &ast);
        if (gather && rc == MCRT_OK) rc = set_gather();
        auto dump = [&](const std::string& path, const void* data, size_t bytes) {
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(data, 1, bytes, o) == bytes;
            if (o) std::fclose(o);
            if (!ok) std::fprintf(stderr, "cannot write %s\n", path.c_str());
            return ok;
        };
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        if (!aov.empty()) {
            if (!(dump(aov + ".depth.f64", depth.data(), px * 8) && dump(aov + ".position.f64", position.data(), px * 24) &&
                  dump(aov + ".normal.f64", normal.data(), px * 24) && dump(aov + ".shading_normal.f64", shading_normal.data(), px * 24) &&
                  dump(aov + ".albedo.f64", albedo.data(), px * 24) && dump(aov + ".coverage.f64", coverage.data(), px * 8) &&
                  dump(aov + ".surface.u32", surface.data(), px * 4) && dump(aov + ".material.u32", material.data(), px * 4)))
                return 1;
            std::printf("{\"aov\":\"%s\",\"rays\":%llu,\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"Mray_s\":%.1f}\n", aov.c_str(), (unsigned long long)ast.rays,
                        ast.kernel_ms, ast.total_ms, ast.rays / ast.kernel_ms / 1e3);
        }
        if (!denoise.empty()) {
            std::vector<double> filtered(px * 3);
            mcrt_stats dst;
            rc = mcrt_denoise(ctx, cam.width, cam.height, rgb.data(), &b, &dparams, filtered.data(), &dst);
            if (rc != MCRT_OK) {
                std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
                return 1;
            }
            if (!dump(denoise, filtered.data(), px * 24)) return 1;
            std::printf("{\"denoise\":\"%s\",\"kernel_launches\":%u,\"kernel_ms\":%.3f,\"total_ms\":%.3f}\n", denoise.c_str(), dst.kernel_launches,
                        dst.kernel_ms, dst.total_ms);
            if (!compare_frame("denoise", filtered, false)) return 1;
            if (!tga.empty()) {
                const size_t dot = denoise.find_last_of('.'), slash = denoise.find_last_of('/');
                const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
                if (!develop(filtered, (has_ext ? denoise.substr(0, dot) : denoise) + ".tga")) return 1;
            }
            if (!exr.empty()) exr_layer("denoise", "RGB", exr_keep(filtered), MCRT_EXR_HALF);
        }
        if (!dvar.empty()) {
            std::vector<double> filtered(px * 3), filtered_var(px * 3);
            mcrt_denoise_variance_params vparams{};
            vparams.iterations = dparams.iterations;
            mcrt_stats dst;
            mcrt_frame_noise_result raw, fn;
            rc = mcrt_denoise_variance(ctx, cam.width, cam.height, spp, rgb.data(), variance.data(), &b, &vparams, filtered.data(), filtered_var.data(), &dst);
            if (rc == MCRT_OK) rc = mcrt_frame_noise(ctx, px, spp, rgb.data(), variance.data(), &raw);
            if (rc == MCRT_OK) rc = mcrt_frame_noise(ctx, px, spp, filtered.data(), filtered_var.data(), &fn);
            if (rc != MCRT_OK) {
                std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
                return 1;
            }
            if (!dump(dvar, filtered.data(), px * 24)) return 1;
            if (!dvar_out.empty() && !dump(dvar_out, filtered_var.data(), px * 24)) return 1;
            std::printf("{\"denoise_variance\":\"%s\",\"kernel_launches\":%u,\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"relative_error_raw\":%.17g,"
                        "\"relative_error\":%.17g}\n",
                        dvar.c_str(), dst.kernel_launches, dst.kernel_ms, dst.total_ms, raw.relative_error, fn.relative_error);
            if (!compare_frame("denoise_variance", filtered, false)) return 1;
            if (!tga.empty()) {
                const size_t dot = dvar.find_last_of('.'), slash = dvar.find_last_of('/');
                const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
                if (!develop(filtered, (has_ext ? dvar.substr(0, dot) : dvar) + ".tga")) return 1;
            }
            if (!exr.empty()) {
                exr_layer("denoise_variance", "RGB", exr_keep(filtered), MCRT_EXR_HALF);
                exr_layer("denoise_variance.variance", "RGB", exr_keep(filtered_var), MCRT_EXR_FLOAT);
            }
        }
        if (!exr.empty()) {
            exr_layer("depth", "Z", exr_keep(depth), MCRT_EXR_FLOAT, 1);
            exr_layer("position", "XYZ", exr_keep(position), MCRT_EXR_FLOAT);
            exr_layer("normal", "XYZ", exr_keep(normal), MCRT_EXR_HALF);
            exr_layer("shading_normal", "XYZ", exr_keep(shading_normal), MCRT_EXR_HALF);
            exr_layer("albedo", "RGB", exr_keep(albedo), MCRT_EXR_HALF);
            exr_layer("coverage", "A", exr_keep(coverage), MCRT_EXR_HALF, 1);
            exr_one("surface.id", exr_keep_u32(surface), MCRT_EXR_UINT, 1, 0);
            exr_one("material.id", exr_keep_u32(material), MCRT_EXR_UINT, 1, 0);
        }
    }
    if (!matte.empty()) {
        const size_t px = (size_t)cam.width * cam.height;
        const uint32_t ranks = mparams.ranks ? mparams.ranks : MCRT_MATTE_DEFAULT_RANKS;
        if (ranks > MCRT_MATTE_MAX_RANKS) {
            std::fprintf(stderr, "--matte-ranks: %u at most\n", MCRT_MATTE_MAX_RANKS);
            return 2;
        }
        std::vector<uint32_t> id(px * ranks), distinct(px);
        std::vector<double> coverage(px * ranks), layer(exr.empty() ? 0 : px * ranks * 2);
        const mcrt_matte_buffers mb{id.data(), coverage.data(), exr.empty() ? nullptr : layer.data(), distinct.data()};
        mcrt_stats mst;
        rc = mcrt_render_matte(ctx, &cam, seed, &mparams, &mb, nullptr, &mst);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        auto dump = [&](const std::string& path, const void* data, size_t bytes) {
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(data, 1, bytes, o) == bytes;
            if (o) std::fclose(o);
            if (!ok) std::fprintf(stderr, "cannot write %s\n", path.c_str());
            return ok;
        };
        if (!(dump(matte + ".id.u32", id.data(), px * ranks * 4) && dump(matte + ".coverage.f64", coverage.data(), px * ranks * 8) &&
              dump(matte + ".distinct.u32", distinct.data(), px * 4)))
            return 1;
        uint32_t most = 0;
        for (uint32_t d : distinct) most = d > most ? d : most;
        std::printf("{\"matte\":\"%s\",\"key\":\"%s\",\"ranks\":%u,\"max_distinct\":%u,\"rays\":%llu,\"kernel_ms\":%.3f,\"total_ms\":%.3f}\n", matte.c_str(),
                    mparams.key == MCRT_MATTE_SURFACE ? "surface" : "material", ranks, most, (unsigned long long)mst.rays, mst.kernel_ms, mst.total_ms);
        if (!exr.empty()) {
            const std::string name = mparams.key == MCRT_MATTE_SURFACE ? "CryptoSurface" : "CryptoMaterial";
            const double* data = exr_keep(layer);
            for (uint32_t i = 0; i < 2 * ranks; i++) {
                char level[8];
                std::snprintf(level, sizeof level, "%02u", i / 4);
                exr_one(name + level + "." + "RGBA"[i % 4], data, MCRT_EXR_FLOAT, 2 * ranks, i);
            }
            char code[12];
            std::snprintf(code, sizeof code, "%08x", mcrt_matte_code(name.c_str()));
            const std::string key = "cryptomatte/" + std::string(code, 7) + "/";
            const char* said[3][2] = {{"name", name.c_str()}, {"hash", "MurmurHash3_32"}, {"conversion", "uint32_to_float32"}};
            for (const auto& kv : said) {
                exr_attr_text.push_back(key + kv[0]);
                exr_attr_text.push_back(kv[1]);
            }
            const mcrt_scene_desc* sd = mcrt_image_scene(img);
            const uint32_t num_keys = mparams.key == MCRT_MATTE_SURFACE ? sd->num_surfaces : sd->num_materials;
            const int64_t need = mcrt_matte_manifest(&mparams, num_keys, nullptr, 0);
            if (need > 0 && need <= (1 << 20)) {
                std::string text((size_t)need, '\0');
                mcrt_matte_manifest(&mparams, num_keys, &text[0], (uint64_t)need);
                text.resize((size_t)need - 1);
                exr_attr_text.push_back(key + "manifest");
                exr_attr_text.push_back(text);
            } else {
                std::fprintf(stderr, "--matte: the manifest of %u names would take %lld bytes: left out of %s\n", num_keys, (long long)need, exr.c_str());
            }
        }
    }
    if (!occlusion.empty()) {
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<double> ao(px), sky(px), bent(px * 3);
        const mcrt_occlusion_buffers ob{ao.data(), sky.data(), bent.data()};
        mcrt_stats ost;
        rc = mcrt_render_occlusion(ctx, &cam, seed, &oparams, &ob, &ost);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        auto dump = [&](const std::string& path, const void* data, size_t bytes) {
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(data, 1, bytes, o) == bytes;
            if (o) std::fclose(o);
            if (!ok) std::fprintf(stderr, "cannot write %s\n", path.c_str());
            return ok;
        };
        if (!(dump(occlusion + ".ao.f64", ao.data(), px * 8) && dump(occlusion + ".sky.f64", sky.data(), px * 8) && dump(occlusion + ".bent_normal.f64", bent.data(), px * 24)))
            return 1;
        double mean_ao = 0.0;
        for (double a : ao) mean_ao += a;
        std::printf("{\"occlusion\":\"%s\",\"occlusion_rays\":%u,\"max_distance\":%.17g,\"mean_ao\":%.6f,\"rays\":%llu,\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"Mray_s\":%.1f}\n",
                    occlusion.c_str(), oparams.rays ? oparams.rays : 1u, oparams.max_distance, px ? mean_ao / (double)px : 0.0, (unsigned long long)ost.rays, ost.kernel_ms,
                    ost.total_ms, ost.rays / ost.kernel_ms / 1e3);
        if (!exr.empty()) {
            exr_one("occlusion.ao", exr_keep(ao), MCRT_EXR_HALF, 1, 0);
            exr_one("occlusion.sky", exr_keep(sky), MCRT_EXR_HALF, 1, 0);
            exr_layer("occlusion.bent", "XYZ", exr_keep(bent), MCRT_EXR_HALF);
        }
    }
    if (!lighting.empty()) {
        if (photon) {
            std::fprintf(stderr, "--lighting: the lighting passes are the path tracer's (not with --photon)\n");
            return 1;
        }
        const size_t px = (size_t)cam.width * cam.height;
        static const char* const names[5] = {"emission", "sky", "direct", "light", "unoccluded"};
        std::vector<double> frames[5];
        for (auto& f : frames) f.resize(px * 3);
        const mcrt_lighting_buffers lb{frames[0].data(), frames[1].data(), frames[2].data(), frames[3].data(), frames[4].data()};
        mcrt_stats lst;
        rc = mcrt_render_lighting(ctx, &cam, seed, &lb, &lst);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        double mean[5] = {0, 0, 0, 0, 0};
        for (int c = 0; c < 5; c++) {
            const std::string path = lighting + "." + names[c] + ".f64";
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(frames[c].data(), 1, px * 24, o) == px * 24;
            if (o) std::fclose(o);
            if (!ok) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                return 1;
            }
            for (double w : frames[c]) mean[c] += w;
            mean[c] = px ? mean[c] / (double)(px * 3) : 0.0;
        }
        std::printf("{\"lighting\":\"%s\",\"mean_emission\":%.6g,\"mean_sky\":%.6g,\"mean_direct\":%.6g,\"mean_light\":%.6g,\"mean_unoccluded\":%.6g,\"rays\":%llu,"
                    "\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"Mray_s\":%.1f}\n",
                    lighting.c_str(), mean[0], mean[1], mean[2], mean[3], mean[4], (unsigned long long)lst.rays, lst.kernel_ms, lst.total_ms, lst.rays / lst.kernel_ms / 1e3);
        if (!exr.empty())
            for (int c = 0; c < 5; c++) exr_layer(std::string("lighting.") + names[c], "RGB", exr_keep(frames[c]), MCRT_EXR_HALF);
    }
    if (!light_groups.empty()) {
        if (photon) {
            std::fprintf(stderr, "--light-groups: the light groups are the path tracer's (not with --photon)\n");
            return 1;
        }
        std::vector<uint32_t> group;
        std::vector<std::string> names;
        if (!light_group_map(group, names)) return 1;
        mcrt_light_group_params gp{};
        gp.num_groups = (uint32_t)names.size();
        gp.max_depth = light_groups_depth;
        gp.flags = film.empty() ? 0u : MCRT_LIGHT_GROUPS_FILM;
        gp.surface_group = group.data();
        names.push_back("sky");
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<double> planes(names.size() * px * 3);
        mcrt_stats gst;
        rc = mcrt_render_light_groups(ctx, &cam, seed, &gp, planes.data(), &gst);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        std::string means;
        for (size_t p = 0; p < names.size(); p++) {
            const double* plane = planes.data() + p * px * 3;
            const std::string path = light_groups + "." + names[p] + ".f64";
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(plane, 1, px * 24, o) == px * 24;
            if (o) std::fclose(o);
            if (!ok) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                return 1;
            }
            double mean = 0.0;
            for (size_t w = 0; w < px * 3; w++) mean += plane[w];
            char text[96];
            std::snprintf(text, sizeof text, "%s\"%s\":%.6g", p ? "," : "", names[p].c_str(), px ? mean / (double)(px * 3) : 0.0);
            means += text;
            if (!exr.empty()) {
                std::vector<double> copy(plane, plane + px * 3);
                exr_layer("lightgroup." + names[p], "RGB", exr_keep(copy), MCRT_EXR_HALF);
            }
        }
        std::printf("{\"light_groups\":\"%s\",\"by\":\"%s\",\"max_depth\":%u,\"means\":{%s},\"rays\":%llu,\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"Mray_s\":%.1f}\n",
                    light_groups.c_str(), light_groups_by.c_str(), light_groups_depth, means.c_str(), (unsigned long long)gst.rays, gst.kernel_ms, gst.total_ms,
                    gst.rays / gst.kernel_ms / 1e3);
    }
    if (!path_classes.empty()) {
        if (photon) {
            std::fprintf(stderr, "--path-classes: the path classes are the path tracer's (not with --photon)\n");
            return 1;
        }
        const char* const names[MCRT_PATH_CLASSES] = {"emission",      "background",      "diffuse_direct",      "diffuse_indirect",
                                                      "glossy_direct", "glossy_indirect", "transmission_direct", "transmission_indirect"};
        mcrt_path_class_params pp{};
        pp.max_depth = path_classes_depth;
        pp.flags = film.empty() ? 0u : MCRT_PATH_CLASSES_FILM;
        const size_t px = (size_t)cam.width * cam.height;
        std::vector<double> planes(MCRT_PATH_CLASSES * px * 3);
        mcrt_stats pst;
        rc = mcrt_render_path_classes(ctx, &cam, seed, &pp, planes.data(), &pst);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        std::string means;
        for (size_t p = 0; p < MCRT_PATH_CLASSES; p++) {
            const double* plane = planes.data() + p * px * 3;
            const std::string path = path_classes + "." + names[p] + ".f64";
            FILE* o = std::fopen(path.c_str(), "wb");
            const bool ok = o && std::fwrite(plane, 1, px * 24, o) == px * 24;
            if (o) std::fclose(o);
            if (!ok) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                return 1;
            }
            double mean = 0.0;
            for (size_t w = 0; w < px * 3; w++) mean += plane[w];
            char text[96];
            std::snprintf(text, sizeof text, "%s\"%s\":%.6g", p ? "," : "", names[p], px ? mean / (double)(px * 3) : 0.0);
            means += text;
            if (!exr.empty()) {
                std::vector<double> copy(plane, plane + px * 3);
                exr_layer(std::string("pathclass.") + names[p], "RGB", exr_keep(copy), MCRT_EXR_HALF);
            }
        }
        eparams.flags |= MCRT_EXR_LONG_NAMES;  // (pathclass.transmission_indirect.R is 33 bytes)
        std::printf("{\"path_classes\":\"%s\",\"max_depth\":%u,\"means\":{%s},\"rays\":%llu,\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"Mray_s\":%.1f}\n", path_classes.c_str(),
                    path_classes_depth, means.c_str(), (unsigned long long)pst.rays, pst.kernel_ms, pst.total_ms, pst.rays / pst.kernel_ms / 1e3);
    }
    if (!exr.empty()) {
        const std::string a_spp = std::to_string(spp), a_seed = std::to_string(seed), a_kernel = std::to_string(st.kernel_id);
        std::vector<mcrt_exr_attribute> attributes = {{"mcrt:spp", a_spp.c_str()}, {"mcrt:seed", a_seed.c_str()},
                                                      {"mcrt:integrator", photon ? "photon_mapper" : "path_tracer"}, {"mcrt:kernel", a_kernel.c_str()}};
        for (size_t i = 0; i + 1 < exr_attr_text.size(); i += 2) attributes.push_back({exr_attr_text[i].c_str(), exr_attr_text[i + 1].c_str()});
        mcrt_exr_result er;
        mcrt_stats est;
        rc = mcrt_exr_save(ctx, exr.c_str(), cam.width, cam.height, exr_channels.data(), (uint32_t)exr_channels.size(), attributes.data(), (uint32_t)attributes.size(), &eparams, &er, &est);
        if (rc != MCRT_OK) {
            std::fprintf(stderr, "mcrt error %d: %s\n", rc, mcrt_last_error(ctx));
            return 1;
        }
        std::printf("{\"exr\":\"%s\",\"channels\":%zu,\"file_bytes\":%llu,\"packed_bytes\":%llu,\"chunks\":%u,\"raw_chunks\":%u,\"kernel_ms\":%.3f,\"total_ms\":%.3f}\n",
                    exr.c_str(), exr_channels.size(), (unsigned long long)er.file_bytes, (unsigned long long)er.packed_bytes, er.chunks, er.raw_chunks, est.kernel_ms,
                    est.total_ms);
    }
    std::printf("{\"width\":%u,\"height\":%u,\"spp\":%u,\"paths\":%llu,\"rays\":%llu,\"kernel_ms\":%.3f,\"total_ms\":%.3f,\"Mray_s\":%.1f}\n",
                cam.width, cam.height, spp, (unsigned long long)st.paths, (unsigned long long)st.rays,
                st.kernel_ms, st.total_ms, st.rays / st.kernel_ms / 1e3);
    for (mcrt_ctx* c : ctxs) mcrt_destroy(c);
    mcrt_image_free(img);
    return 0;
}
