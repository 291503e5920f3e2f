// oracle/ref_main.cpp — TEST INFRASTRUCTURE ONLY (never linked into or called by the product path).
//
// Host program that links the UNMODIFIED reference translation units (compiled in place from
// /root/reference/source by oracle/Makefile, with oracle/ref_seed_pin.hpp force-included) and
//   1. "flatten": walks the reference's Scene / BVH / LinearOctree / Camera objects and writes the
//      scene image (*.mcrt) that include/mcrt.h's descriptors describe — this is exactly the
//      flattener a maintainer adds to the reference host;
//   2. "render":  runs the reference's own Camera::samplePixel (camera/camera.cpp:66-99) over a row
//      range with the reference's 32x32 bucket work split and dumps camera.film.scan(x,y) as FP64
//      (the value Camera::sampleImage stores into camera.image, camera.cpp:138-144), timing only
//      the worker section (the reference's own timer is quantised to 1 s, camera.cpp:131,224);
//   3. "kat":     calls individual reference functions on seeded random inputs and dumps
//      known-answer vectors (the reference has no tests of its own);
//   4. "bsdf":    the kat mode's lobe-function rows (Fresnel / GGX / Oren-Nayar) on inputs read from files:
//      the edge vectors of tests/golden/make_bsdf_edges.py.
//
// Private members are reached with -fno-access-control (this TU only; layout is unaffected).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <thread>
#include <unordered_map>

#include <glm/glm.hpp>
#include <glm/gtx/norm.hpp>
#include <nlohmann/json.hpp>

#include "bvh/bvh.hpp"
#include "camera/camera.hpp"
#include "common/coordinate-system.hpp"
#include "common/option.hpp"
#include "integrator/integrator.hpp"
#include "integrator/path-tracer/path-tracer.hpp"
#include "integrator/photon-mapper/photon-mapper.hpp"
#include "material/fresnel.hpp"
#include "material/ggx.hpp"
#include "material/material.hpp"
#include "octree/linear-octree.cpp"  // template bodies (the reference includes them the same way)
#include "octree/octree.cpp"
#include "ray/interaction.hpp"
#include "sampling/sampler.hpp"
#include "sampling/sampling.hpp"
#include "scene/scene.hpp"
#include "surface/surface.hpp"

#include "../include/mcrt.h"
#include "../integration/ref_flatten.hpp"

namespace {

struct Args {
    std::string mode, scene, out, out_samples, out_radiance, out_kat, consts, in;
    int camera = 0;
    bool photon = false;
    long width = -1, height = -1, sqrtspp = -1, threads = -1;
    long row0 = 0, row1 = -1;
    double emissions = -1, caustic_factor = -1, f_stop = 0, focus_distance = 0;
    std::string film_filter;  // camera "film": {"filter", "radius", "cache_size"} (camera.cpp:34-35, film.cpp:19-58)
    double film_radius = 0;
    int film_cache = 0;
    long knn_k = -1;
    std::string bvh;
    long bins = -1;
    long n = 100000;
    std::vector<std::pair<std::string, double>> rough;  // material specular_roughness overrides
    // Image::save (camera/image.cpp:37-52) of the rendered frame: base name (".tga" is appended) and overrides of the
    // camera's "image" object as key=value[,key=value...] ("" = the scene file's values)
    std::vector<std::pair<std::string, std::string>> saves;
    nlohmann::json image_json;  // the camera's "image" object after --width/--height (filled by loadScene)
};

[[noreturn]] void usage() {
    std::fprintf(stderr,
        "usage: mcrt_ref <flatten|render|kat>[,<mode>...] --scene file.json [--camera N] [--photon]\n"
        "   [--width W --height H --sqrtspp S] [--bvh octree|binary_sah|quaternary_sah] [--bins B]\n"
        "   [--threads T] [--rows y0 y1] [--emissions E] [--caustic-factor F] [--k K] [--f-stop X] [--focus-distance D]\n"
        "   [--film-filter mitchell-netravali|catmull-rom|b-spline|hermite|gaussian|lanczos] [--film-radius R] [--film-cache N]\n"
        "   [--specular-roughness material value]... [--n N]\n"
        "   [--save base key=value,...]... (render of the full frame: Image::save to base.tga; keys of the \"image\" object, \"-\" = none)\n"
        "   --out image.mcrt (flatten) --out-radiance file.f64 [--out-samples file.f64] (render) --out-kat dir (kat)\n"
        "   mcrt_ref bsdf --consts consts.f64 --in in.f64 --out out.f64 (the kat mode's lobe-function rows on given inputs; no scene)\n"
        "   several modes in one run share ONE Camera/Scene/photon map (photon order is thread-dependent)\n");
    std::exit(2);
}

Args parse(int argc, char** argv) {
    Args a;
    if (argc < 2) usage();
    a.mode = argv[1];
    for (int i = 2; i < argc; i++) {
        std::string k = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) usage(); return argv[++i]; };
        if (k == "--scene") a.scene = next();
        else if (k == "--out") a.out = next();
        else if (k == "--out-samples") a.out_samples = next();
        else if (k == "--out-radiance") a.out_radiance = next();
        else if (k == "--out-kat") a.out_kat = next();
        else if (k == "--consts") a.consts = next();
        else if (k == "--in") a.in = next();
        else if (k == "--camera") a.camera = std::stoi(next());
        else if (k == "--photon") a.photon = true;
        else if (k == "--width") a.width = std::stol(next());
        else if (k == "--height") a.height = std::stol(next());
        else if (k == "--sqrtspp") a.sqrtspp = std::stol(next());
        else if (k == "--threads") a.threads = std::stol(next());
        else if (k == "--rows") { a.row0 = std::stol(next()); a.row1 = std::stol(next()); }
        else if (k == "--emissions") a.emissions = std::stod(next());
        else if (k == "--caustic-factor") a.caustic_factor = std::stod(next());
        else if (k == "--k") a.knn_k = std::stol(next());
        else if (k == "--f-stop") a.f_stop = std::stod(next());
        else if (k == "--focus-distance") a.focus_distance = std::stod(next());
        else if (k == "--film-filter") a.film_filter = next();
        else if (k == "--film-radius") a.film_radius = std::stod(next());
        else if (k == "--film-cache") a.film_cache = std::stoi(next());
        else if (k == "--bvh") a.bvh = next();
        else if (k == "--bins") a.bins = std::stol(next());
        else if (k == "--n") a.n = std::stol(next());
        else if (k == "--save") { std::string b = next(); a.saves.push_back({b, next()}); }
        else if (k == "--specular-roughness") { std::string m = next(); a.rough.push_back({m, std::stod(next())}); }
        else usage();
    }
    if (a.mode == "bsdf") { if (a.consts.empty() || a.in.empty() || a.out.empty()) usage(); return a; }
    if (a.scene.empty()) usage();
    // single-mode shorthand: --out names that mode's output
    if (a.mode == "render" && a.out_radiance.empty()) a.out_radiance = a.out;
    if (a.mode == "kat" && a.out_kat.empty()) a.out_kat = a.out;
    return a;
}

nlohmann::json loadScene(Args& a) {
    std::ifstream f(a.scene);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", a.scene.c_str()); std::exit(1); }
    nlohmann::json j;
    f >> j;
    auto& cam = j.at("cameras").at(a.camera);
    if (a.width > 0) cam["image"]["width"] = a.width;
    if (a.height > 0) cam["image"]["height"] = a.height;
    if (a.sqrtspp > 0) cam["sqrtspp"] = a.sqrtspp;
    if (a.f_stop != 0) cam["f_stop"] = a.f_stop;                       // thin lens (camera.cpp:41-42,63)
    if (a.focus_distance != 0) cam["focus_distance"] = a.focus_distance;
    if (!a.film_filter.empty()) {
        cam["film"] = {{"filter", a.film_filter}};
        if (a.film_radius > 0) cam["film"]["radius"] = a.film_radius;
        if (a.film_cache > 0) cam["film"]["cache_size"] = a.film_cache;
    }
    if (a.threads > 0) j["num_render_threads"] = a.threads;
    if (!a.bvh.empty()) {
        if (a.bvh == "none") j.erase("bvh");
        else j["bvh"] = {{"type", a.bvh}};
        if (a.bins > 0 && a.bvh != "none") j["bvh"]["bins_per_axis"] = a.bins;
    }
    if (a.emissions > 0) j["photon_map"]["emissions"] = a.emissions;
    if (a.caustic_factor > 0) j["photon_map"]["caustic_factor"] = a.caustic_factor;
    if (a.knn_k > 0) j["photon_map"]["k_nearest_photons"] = a.knn_k;
    for (const auto& r : a.rough) j["materials"][r.first]["specular_roughness"] = r.second;
    Scene::path = std::filesystem::absolute(std::filesystem::path(a.scene)).parent_path();
    a.image_json = cam.at("image");
    return j;
}

// ---------------------------------------------------------------------------------------------
// flatten: integration/ref_flatten.hpp (Flat, FlatMap, flattenScene, flattenMap, flattenCamera)
// ---------------------------------------------------------------------------------------------
void writeRaw(const std::string& path, const void* data, size_t nbytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, 1, nbytes, f) != nbytes) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
    std::fclose(f);
}

int doFlatten(const Args& a, Camera& camera) {
    Flat F;
    flattenScene(camera.integrator->scene, F);
    mcrt_camera_desc cd = flattenCamera(camera);
    FlatMap G, C;
    const mcrt_photon_map_desc *gp = nullptr, *cp = nullptr;
    std::vector<const char*> keys = {"global_seed", "photon_mapping"};
    std::vector<uint64_t> vals = {Sampler::global_seed, a.photon ? 1u : 0u};
    if (auto pm = dynamic_cast<PhotonMapper*>(camera.integrator.get())) {
        flattenMap(pm->global_map, G);
        flattenMap(pm->caustic_map, C);
        if (G.desc.num_octants) gp = &G.desc;
        if (C.desc.num_octants) cp = &C.desc;
        keys.push_back("k_nearest_photons"); vals.push_back(pm->k_nearest_photons);
        keys.push_back("direct_visualization"); vals.push_back(pm->direct_visualization ? 1 : 0);
    }
    {   // the camera's "image" object (image.cpp:17-34) for hosts that develop the frame with mcrt_tonemap; doubles as bit patterns
        const Image& im = camera.image;
        std::string tm = getOptional<std::string>(a.image_json, "tonemapper", "HABLE");
        std::transform(tm.begin(), tm.end(), tm.begin(), toupper);
        auto bits = [](double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; };
        keys.push_back("image_tonemapper"); vals.push_back(tm == "ACES" ? MCRT_TONEMAP_ACES : MCRT_TONEMAP_HABLE);
        keys.push_back("image_plain"); vals.push_back(im.plain ? 1 : 0);
        keys.push_back("image_exposure_ev_bits"); vals.push_back(bits(getOptional(a.image_json, "exposure_compensation", 0.0)));
        keys.push_back("image_gain_ev_bits"); vals.push_back(bits(getOptional(a.image_json, "gain_compensation", 0.0)));
    }
    int rc = mcrt_image_save(a.out.c_str(), &F.desc, &cd, gp, cp, keys.data(), vals.data(), (uint32_t)keys.size());
    std::printf("flatten: %u nodes, %u surfaces, %u materials, %u lights, photons g=%llu c=%llu -> %s (rc=%d)\n",
                F.desc.num_nodes, F.desc.num_surfaces, F.desc.num_materials, F.desc.num_lights,
                (unsigned long long)G.desc.num_photons, (unsigned long long)C.desc.num_photons, a.out.c_str(), rc);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// render (reference Camera::samplePixel over a row range)
// ---------------------------------------------------------------------------------------------
int doRender(const Args& a, Camera& camera) {
    const long W = (long)camera.image.width, H = (long)camera.image.height;
    long y0 = a.row0, y1 = a.row1 < 0 ? H : std::min(a.row1, H);
    const long B = 32;  // Camera::bucket_size (camera/camera.hpp:68)
    struct Bucket { long x0, x1, y0, y1; };
    std::vector<Bucket> buckets;
    for (long x = 0; x < W; x += B)
        for (long y = y0; y < y1; y += B)
            buckets.push_back({x, std::min(x + B, W), y, std::min(y + B, y1)});
    std::atomic<size_t> next{0};
    size_t nthreads = camera.integrator->num_threads;

    std::vector<double> samples;
    const size_t spp = camera.sqrtspp * camera.sqrtspp;
    const bool per_sample = !a.out_samples.empty();
    if (per_sample) samples.assign((size_t)W * (y1 - y0) * spp * 3, 0.0);

    auto worker = [&]() {
        size_t b;
        while ((b = next.fetch_add(1)) < buckets.size()) {
            const Bucket& k = buckets[b];
            for (long y = k.y0; y < k.y1; y++)
                for (long x = k.x0; x < k.x1; x++) {
                    if (!per_sample) {
                        camera.samplePixel((size_t)x, (size_t)y);
                    } else {
                        // Same statements as Camera::samplePixel (camera.cpp:66-99), but keeping each
                        // sample's radiance; pinhole only (asserted below).
                        double pixel_size = camera.sensor_width / camera.image.width;
                        glm::dvec2 half_dim = glm::dvec2(camera.image.width, camera.image.height) * 0.5;
                        Sampler::initiate(static_cast<uint32_t>(y * camera.image.width + x));
                        for (size_t i = 0; i < spp; i++) {
                            Sampler::setIndex((uint32_t)i);
                            auto u = Sampler::get<Dim::PIXEL, 2>();
                            glm::dvec2 px(x + u[0], y + u[1]);
                            glm::dvec2 local = pixel_size * (half_dim - px);
                            glm::dvec3 direction = glm::normalize(camera.forward * camera.focal_length + camera.left * local.x + camera.up * local.y);
                            Ray ray(camera.eye, direction, camera.integrator->scene.ior);
                            glm::dvec3 L = camera.integrator->sampleRay(ray);
                            camera.film.deposit(px, L);
                            double* o = &samples[(((size_t)(y - y0) * W + x) * spp + i) * 3];
                            o[0] = L.x; o[1] = L.y; o[2] = L.z;
                        }
                    }
                }
        }
    };
    if (per_sample && camera.thin_lens) { std::fprintf(stderr, "--out-samples supports pinhole cameras only\n"); return 3; }

    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nthreads; t++) pool.emplace_back(worker);
    for (auto& t : pool) t.join();
    auto t1 = std::chrono::steady_clock::now();
    double sec = std::chrono::duration<double>(t1 - t0).count();

    std::vector<double> out((size_t)W * (y1 - y0) * 3);
    for (long y = y0; y < y1; y++)
        for (long x = 0; x < W; x++) {
            glm::dvec3 c = camera.film.scan((size_t)x, (size_t)y);
            double* o = &out[((size_t)(y - y0) * W + x) * 3];
            o[0] = c.x; o[1] = c.y; o[2] = c.z;
        }
    writeRaw(a.out_radiance, out.data(), out.size() * sizeof(double));
    if (per_sample) writeRaw(a.out_samples, samples.data(), samples.size() * sizeof(double));
    // Camera::saveImage's copy (camera.cpp:138-143) + Image::save, once per --save with that "image" object
    std::string saves = "[";
    for (const auto& sv : a.saves) {
        if (y0 != 0 || y1 != H) { std::fprintf(stderr, "--save needs the full frame\n"); return 3; }
        nlohmann::json ij = a.image_json;
        std::stringstream ss(sv.second == "-" ? std::string() : sv.second);
        for (std::string kv; std::getline(ss, kv, ',');) {
            auto eq = kv.find('=');
            std::string key = kv.substr(0, eq), val = kv.substr(eq + 1);
            if (key == "tonemapper") ij[key] = val;
            else if (key == "plain") ij[key] = (val == "true" || val == "1");
            else ij[key] = std::stod(val);
        }
        Image im(ij);
        for (long y = 0; y < H; y++)
            for (long x = 0; x < W; x++) im((size_t)x, (size_t)y) = camera.film.scan((size_t)x, (size_t)y);
        im.save(sv.first);
        double ef = im.plain ? 1.0 : im.getExposure() * im.exposure_scale;
        double gf = im.plain ? 1.0 : im.getGain(ef) * im.gain_scale;
        std::string tm = getOptional<std::string>(ij, "tonemapper", "HABLE");
        std::transform(tm.begin(), tm.end(), tm.begin(), toupper);
        char buf[512];
        std::snprintf(buf, sizeof buf, "%s{\"tonemapper\":\"%s\",\"plain\":%s,\"exposure_compensation\":%.17g,\"gain_compensation\":%.17g,"
                      "\"exposure_factor\":%.17g,\"gain_factor\":%.17g}", saves.size() > 1 ? "," : "", tm == "ACES" ? "ACES" : "HABLE",
                      im.plain ? "true" : "false", getOptional(ij, "exposure_compensation", 0.0), getOptional(ij, "gain_compensation", 0.0), ef, gf);
        saves += buf;
    }
    saves += "]";
    double paths = (double)W * (y1 - y0) * spp;
    std::printf("{\"mode\":\"render\",\"saves\":%s,", saves.c_str());
    std::printf("\"width\":%ld,\"rows\":[%ld,%ld],\"spp\":%zu,\"threads\":%zu,"
                "\"paths\":%.0f,\"seconds\":%.6f,\"paths_per_s\":%.1f,\"seed\":%u}\n",
                W, y0, y1, spp, nthreads, paths, sec, paths / sec, Sampler::global_seed);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// kat: known-answer vectors from individual reference functions
// ---------------------------------------------------------------------------------------------
struct Rng {  // splitmix64; the tests regenerate the same inputs from the dumped arrays, not from this
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (next() >> 11) * 0x1p-53; }
    double range(double a, double b) { return a + (b - a) * uni(); }
};

glm::dvec3 randDir(Rng& r) {
    double z = r.range(-1, 1), phi = r.range(0, 6.283185307179586);
    double s = std::sqrt(1 - z * z);
    return glm::dvec3(s * std::cos(phi), s * std::sin(phi), z);
}

// One row of the lobe-function vectors, for doKat's seeded inputs and for doBsdf's inputs from a file alike.
// in: wi(3) wo(3) n1 n2 alpha u v | out: F_dielectric, conductor(3), GGX refl (f,pdf), GGX trans (f,pdf),
//     visibleMicrofacet(3), D(m), Lambda(wo), OrenNayar-diffuse (rgb, pdf)
// consts: roughness, reflectance(3) of the diffuse material (rough as Material::computeProperties decides), complex IOR real(3), imaginary(3)
struct BsdfKat {
    Material rough_mat;
    ComplexIOR cior;
    explicit BsdfKat(const double* c) : cior(glm::dvec3(c[4], c[5], c[6]), glm::dvec3(c[7], c[8], c[9])) {
        rough_mat.roughness = c[0]; rough_mat.reflectance = glm::dvec3(c[1], c[2], c[3]);
        rough_mat.computeProperties();
    }
    void row(const double* I, double* O) {
        const glm::dvec3 wi(I[0], I[1], I[2]), wo(I[3], I[4], I[5]);
        const double n1 = I[6], n2 = I[7], alpha = I[8], u = I[9], v = I[10];
        glm::dvec2 al(alpha);
        O[0] = Fresnel::dielectric(n1, n2, wo.z);
        glm::dvec3 fc = Fresnel::conductor(n1, &cior, wo.z);
        O[1] = fc.x; O[2] = fc.y; O[3] = fc.z;
        glm::dvec3 wir = wi; wir.z = std::abs(wir.z) + 1e-3; wir = glm::normalize(wir);
        double pdf;
        O[4] = GGX::reflection(wir, wo, al, pdf); O[5] = pdf;
        glm::dvec3 wit = -wir;
        O[6] = GGX::transmission(wit, wo, n1, n2, al, pdf); O[7] = pdf;
        glm::dvec3 m = GGX::visibleMicrofacet(u, v, wo, al);
        O[8] = m.x; O[9] = m.y; O[10] = m.z;
        O[11] = GGX::D(m, al);
        O[12] = GGX::Lambda(wo, al);
        glm::dvec3 d = rough_mat.diffuseReflection(wir, wo, pdf);
        O[13] = d.x; O[14] = d.y; O[15] = d.z; O[16] = pdf;
        O[17] = 0.0;
    }
};

// bsdf: the same rows on inputs read from files (no scene): consts[10] and in[n][11] -> out[n][18], raw FP64
std::vector<double> readDoubles(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(1); }
    std::vector<double> v((size_t)f.tellg() / sizeof(double));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(double)));
    return v;
}

int doBsdf(const Args& a) {
    const std::vector<double> consts = readDoubles(a.consts), in = readDoubles(a.in);
    if (consts.size() != 10 || in.empty() || in.size() % 11) { std::fprintf(stderr, "bsdf: --consts holds 10 doubles, --in 11 per row\n"); return 2; }
    const size_t n = in.size() / 11;
    std::vector<double> out(n * 18);
    BsdfKat kat(consts.data());
    for (size_t i = 0; i < n; i++) kat.row(&in[i * 11], &out[i * 18]);
    writeRaw(a.out, out.data(), out.size() * 8);
    std::printf("bsdf: %zu rows -> %s\n", n, a.out.c_str());
    return 0;
}

int doKat(const Args& a, Camera& camera) {
    std::string dir = a.out_kat;
    std::filesystem::create_directories(dir);
    const Scene& scene = camera.integrator->scene;
    Flat F;
    flattenScene(scene, F);
    const size_t N = (size_t)a.n;
    Rng rng(0xC0FFEE);

    {   // Sampler (sampling/sampler.hpp): (pixel, index, shuffles) -> get<0,7>()
        const size_t n = 4096;
        std::vector<uint32_t> in(n * 3);
        std::vector<double> out(n * 7);
        for (size_t i = 0; i < n; i++) {
            uint32_t pixel = i < 8 ? (uint32_t[]){0, 0, 0, 12345, 2073599, 1, 65535, 0xFFFFFFFFu}[i] : (uint32_t)(rng.next() % 8294400ull);
            uint32_t index = i < 8 ? (uint32_t[]){0, 1, 255, 0, 1, 1023, 7, 0xFFFFFFFFu}[i] : (uint32_t)(rng.next() % 1024ull);
            uint32_t shuffles = (uint32_t)(i % 5);
            in[i * 3] = pixel; in[i * 3 + 1] = index; in[i * 3 + 2] = shuffles;
            Sampler::initiate(pixel);
            Sampler::setIndex(index);
            for (uint32_t s = 0; s < shuffles; s++) Sampler::shuffle();
            auto u = Sampler::get<0, 7>();
            for (int d = 0; d < 7; d++) out[i * 7 + d] = u[d];
        }
        writeRaw(dir + "/sampler_in.u32", in.data(), in.size() * 4);
        writeRaw(dir + "/sampler_out.f64", out.data(), out.size() * 8);
    }
    {   // Scene::intersect (scene/scene.cpp:151-176) on random rays
        BoundingBox bb = scene.BB();
        std::vector<double> rays(N * 6), t(N), uv(N * 2);
        std::vector<uint32_t> surf(N);
        for (size_t i = 0; i < N; i++) {
            glm::dvec3 o(rng.range(bb.min.x, bb.max.x), rng.range(bb.min.y, bb.max.y), rng.range(bb.min.z, bb.max.z));
            glm::dvec3 d = randDir(rng);
            if (i % 7 == 0) { o = camera.eye; }
            if (i % 97 == 0) { d = glm::dvec3(0); d[(i / 97) % 3] = (i & 1) ? 1.0 : -1.0; }  // axis-parallel: inf/NaN slabs
            Ray ray(o, d, 1.0);
            Intersection is = scene.intersect(ray);
            for (int c = 0; c < 3; c++) { rays[i * 6 + c] = o[c]; rays[i * 6 + 3 + c] = d[c]; }
            t[i] = is.t;
            surf[i] = is ? F.index.at(is.surface.get()) : 0xFFFFFFFFu;
            uv[i * 2] = is.interpolate ? is.uv.x : 0.0;
            uv[i * 2 + 1] = is.interpolate ? is.uv.y : 0.0;
        }
        writeRaw(dir + "/isect_rays.f64", rays.data(), rays.size() * 8);
        writeRaw(dir + "/isect_t.f64", t.data(), t.size() * 8);
        writeRaw(dir + "/isect_surface.u32", surf.data(), surf.size() * 4);
        writeRaw(dir + "/isect_uv.f64", uv.data(), uv.size() * 8);
    }
    {   // Fresnel / GGX / Material lobes on random local-frame directions.
        // in: wi(3) wo(3) n1 n2 alpha u v | out: F_dielectric, conductor(3), GGX refl (f,pdf), GGX trans (f,pdf),
        //     visibleMicrofacet(3), D(m), Lambda(wo), OrenNayar-diffuse (rgb, pdf)
        const size_t n = std::min<size_t>(N, 20000);
        std::vector<double> in(n * 11), out(n * 18);
        const double consts[10] = {0.7, 0.8, 0.6, 0.4, 0.27, 0.68, 1.32, 3.6, 2.6, 2.3};
        BsdfKat kat(consts);
        writeRaw(dir + "/bsdf_consts.f64", consts, 80);
        for (size_t i = 0; i < n; i++) {
            glm::dvec3 wo = randDir(rng); wo.z = std::abs(wo.z) + 1e-3; wo = glm::normalize(wo);
            glm::dvec3 wi = randDir(rng);
            double n1 = (i & 1) ? 1.0 : rng.range(1.0, 2.5), n2 = rng.range(1.0, 3.5);
            double alpha = rng.range(0.01, 0.9), u = rng.uni(), v = rng.uni();
            double* I = &in[i * 11];
            I[0] = wi.x; I[1] = wi.y; I[2] = wi.z; I[3] = wo.x; I[4] = wo.y; I[5] = wo.z;
            I[6] = n1; I[7] = n2; I[8] = alpha; I[9] = u; I[10] = v;
            kat.row(I, &out[i * 18]);
        }
        writeRaw(dir + "/bsdf_in.f64", in.data(), in.size() * 8);
        writeRaw(dir + "/bsdf_out.f64", out.data(), out.size() * 8);
    }
    if (auto pm = dynamic_cast<PhotonMapper*>(camera.integrator.get())) {
        // LinearOctree<Photon>::knnSearch (octree/linear-octree.cpp:25-117)
        const size_t n = std::min<size_t>(N, 20000);
        const size_t k = pm->k_nearest_photons;
        BoundingBox bb = scene.BB();
        for (int which = 0; which < 2; which++) {
            const LinearOctree<Photon>& map = which ? pm->caustic_map : pm->global_map;
            if (map.linear_tree.empty()) continue;
            std::vector<double> pts(n * 3), d2(n * k, std::numeric_limits<double>::infinity());
            std::vector<uint32_t> cnt(n), idx(n * k, 0xFFFFFFFFu);
            PriorityQueue<SearchResult<Photon>> res;
            for (size_t i = 0; i < n; i++) {
                glm::dvec3 p(rng.range(bb.min.x, bb.max.x), rng.range(bb.min.y, bb.max.y), rng.range(bb.min.z, bb.max.z));
                if (i % 3 == 0) {  // near a stored photon (the realistic query)
                    const Photon& ph = map.ordered_data[rng.next() % map.ordered_data.size()];
                    p = ph.pos() + glm::dvec3(rng.range(-0.05, 0.05), rng.range(-0.05, 0.05), rng.range(-0.05, 0.05));
                }
                for (int c = 0; c < 3; c++) pts[i * 3 + c] = p[c];
                map.knnSearch(p, k, res);
                // identify photons by their position in ordered_data via exact distance + payload match
                std::vector<std::pair<double, uint32_t>> found;
                for (const auto& r : res) {
                    // linear probe over candidates is too slow; recover index by pointer arithmetic on payload equality
                    found.push_back({r.distance2, 0});
                }
                // brute-force exact k-NN gives the same set (ties measure zero); indices from brute force
                std::vector<std::pair<double, uint32_t>> all;
                double worst = 0;
                for (const auto& f : found) worst = std::max(worst, f.first);
                for (size_t q = 0; q < map.ordered_data.size(); q++) {
                    double dd = glm::distance2(map.ordered_data[q].pos(), p);
                    if (dd <= worst) all.push_back({dd, (uint32_t)q});
                }
                std::sort(all.begin(), all.end());
                std::sort(found.begin(), found.end());
                if (all.size() != found.size()) {
                    std::fprintf(stderr, "kat knn: reference returned %zu, brute force within radius %zu (query %zu)\n", found.size(), all.size(), i);
                }
                cnt[i] = (uint32_t)found.size();
                for (size_t q = 0; q < found.size() && q < k; q++) {
                    d2[i * k + q] = found[q].first;
                    idx[i * k + q] = q < all.size() ? all[q].second : 0xFFFFFFFFu;
                }
            }
            std::string tag = which ? "c" : "g";
            writeRaw(dir + "/knn_" + tag + "_points.f64", pts.data(), pts.size() * 8);
            writeRaw(dir + "/knn_" + tag + "_count.u32", cnt.data(), cnt.size() * 4);
            writeRaw(dir + "/knn_" + tag + "_index.u32", idx.data(), idx.size() * 4);
            writeRaw(dir + "/knn_" + tag + "_d2.f64", d2.data(), d2.size() * 8);
        }
    }
    std::printf("kat: wrote vectors to %s\n", dir.c_str());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    Args a = parse(argc, argv);
    try {
        if (a.mode == "bsdf") return doBsdf(a);
        nlohmann::json j = loadScene(a);
        Camera camera(j, Option(a.scene, "", a.camera, a.photon));
        int rc = 0, did = 0;
        auto has = [&](const char* m) { return ("," + a.mode + ",").find(std::string(",") + m + ",") != std::string::npos; };
        if (has("flatten")) { if (a.out.empty()) usage(); rc |= doFlatten(a, camera); did++; }
        if (has("kat")) { if (a.out_kat.empty()) usage(); rc |= doKat(a, camera); did++; }
        if (has("render")) { if (a.out_radiance.empty()) usage(); rc |= doRender(a, camera); did++; }
        if (!did) usage();
        return rc;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "mcrt_ref: %s\n", ex.what());
        return 1;
    }
}
