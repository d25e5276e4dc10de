/*
 * ref_shade.cpp — TEST INFRASTRUCTURE.  Harness around the other half of the reference's OWN hot path: include/random_utils.h
 * (wang_hash, random_float, random_in_unit_sphere, random_unit_vector, random_in_hemisphere), include/materials.h (reflectance,
 * material_scatter, material_emit, tex2D_cpu), include/camera.cuh (CameraData::get_ray) and src/camera.cu
 * (Camera::build_camera_data, ray_color_host, Camera::render_cpu, BinarySaver::writeColor) — #included from where they lie under
 * /root/reference (never copied into this repo) and compiled host-only, with the flags of ref_geom.cpp plus -Ishim: the two
 * vendor SDK headers those files name (<curand_kernel.h>, <cuda_runtime.h>) are found as oracle/shim/, alias headers of our own
 * that define no behaviour.  Only the reference's CPU path runs (render_cpu / ray_color_host, what DESIGN.md §1 names as the
 * oracle's subject); no CUDA or HIP runtime function is ever called.
 *
 * Out of scope: src/main.cu — the config parser, the texture loading / CUDA texture upload, and through them the frame loop's
 * camera path (cpu_render's orbit arithmetic is in camera.cu but needs main.cu's SceneParams filled; it is not driven here).
 *
 * Scenes arrive as the arrays the host mirror takes (spheres (cx, cy, cz, radius, material), planes (base, u, v, material, type),
 * materials as 64-byte records of plain fields, textures as float RGBA rows); the harness builds SphereData / PlaneData with the
 * reference's constructors, the tree with the reference's build_bvh and MaterialData field by field (+ an optional CpuTexture).
 * tests/test_ref_shade.py drives the same inputs through this library and through the oracle's orc_shade_* views, bit for bit;
 * tests/golden/make_ref_shade_golden.py records its outputs as fixtures.
 * Built only where /root/reference exists (oracle/Makefile, target `_ref`); output under oracle/_ref/ (git-ignored).
 */
#include <curand_kernel.h>

#include <cstdint>
#include <cstring>
#include <fstream>
#include <ostream>
#include <vector>

#include "vec3.h"
#include "bvh_builder.h"
#include "../src/camera.cu"

// src/camera.cu holds a kernel and two __constant__ symbols, so the host-only object registers them with the GPU runtime when the
// library is loaded — and has no device code to register.  The four registration entry points the compiler's start-up code
// calls are therefore answered here (linked -Bsymbolic), by doing nothing: loading this library never reaches the GPU runtime,
// on a machine with a GPU either.  (The code object symbol that start-up code names is defined as 0 on the link line.)  Hidden: they
// answer this library's own calls and are not exported, so they can never stand in front of the runtime's for anyone else.
#define REF_SHADE_LOCAL extern "C" __attribute__((visibility("hidden")))
REF_SHADE_LOCAL void **__hipRegisterFatBinary(const void *) { static void *none = nullptr; return &none; }
REF_SHADE_LOCAL void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned int, void *, void *, void *, void *, int *) {}
REF_SHADE_LOCAL void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
REF_SHADE_LOCAL void __hipUnregisterFatBinary(void **) {}

namespace {
inline vec3 v(const float *p) { return vec3(p[0], p[1], p[2]); }
inline void put(float *p, const vec3 &a) { p[0] = a[0]; p[1] = a[1]; p[2] = a[2]; }

// a material as plain fields (the layout of rt_material, include/rtp_amd.h): texture = 1-based texture index, 0 = none
struct PlainMaterial {
    int32_t type;
    float fuzz, ir;
    float absorption[3], albedo[3], emit[3];
    uint64_t texture, reserved;
};
MaterialData make_material(const PlainMaterial &m, CpuTexture *textures) {
    MaterialData d;
    d.type = (MaterialType)m.type;
    d.fuzz = m.fuzz;
    d.ir = m.ir;
    d.absorption = v(m.absorption);
    d.albedo = v(m.albedo);
    d.emit = v(m.emit);
    d.tex_obj = 0;
    d.cpu_tex = m.texture ? &textures[m.texture - 1] : nullptr;
    return d;
}
// textures: tex_dims = (offset in floats, width, height) per texture into tex_data
struct RefScene {
    std::vector<SphereData> spheres;
    std::vector<PlaneData> planes;
    std::vector<BVHNode> nodes;
    std::vector<CpuTexture> textures;
    std::vector<MaterialData> materials;
    BVHTree tree;
    SceneData data;
};
void make_scene(RefScene &sc, int32_t ns, const float *spheres5, int32_t np, const float *planes11, int32_t nm, const PlainMaterial *mats,
                int32_t nt, float *tex_data, const int64_t *tex_dims) {
    for (int32_t k = 0; k < ns; ++k) sc.spheres.emplace_back(v(spheres5 + 5 * k), spheres5[5 * k + 3], (int)spheres5[5 * k + 4]);
    for (int32_t k = 0; k < np; ++k) {
        const float *p = planes11 + 11 * k;
        sc.planes.emplace_back(v(p), v(p + 3), v(p + 6), (int)p[9], (PlaneType)(int)p[10]);
    }
    sc.nodes = build_bvh(sc.spheres, sc.planes);
    for (int32_t k = 0; k < nt; ++k) sc.textures.push_back(CpuTexture{tex_data + tex_dims[3 * k], (int)tex_dims[3 * k + 1], (int)tex_dims[3 * k + 2]});
    for (int32_t k = 0; k < nm; ++k) sc.materials.push_back(make_material(mats[k], sc.textures.data()));
    sc.tree.nodes = sc.nodes.data();
    sc.tree.num_nodes = (int)sc.nodes.size();
    sc.data.d_spheres = sc.spheres.data(); sc.data.num_spheres = ns;
    sc.data.d_planes = sc.planes.data(); sc.data.num_planes = np;
    sc.data.d_materials = sc.materials.data(); sc.data.num_materials = nm;
    sc.data.d_bvh_trees = &sc.tree; sc.data.num_bvh_trees = sc.nodes.empty() ? 0 : 1;
}
}  // namespace

extern "C" {

void ref_wang_hash(int64_t n, const uint32_t *in, uint32_t *out) {
    for (int64_t k = 0; k < n; ++k) out[k] = wang_hash(in[k]);
}
void ref_random_float(int64_t n, const uint32_t *seeds, float *out, uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) { unsigned int s = seeds[k]; out[k] = random_float(s); out_seeds[k] = s; }
}
void ref_random_range(int64_t n, const uint32_t *seeds, const float *lo, const float *hi, float *out, uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) { unsigned int s = seeds[k]; out[k] = random_float(s, lo[k], hi[k]); out_seeds[k] = s; }
}
// random_float(seed, -1.0, 1.0) as random_in_unit_sphere writes it: with the double literals
void ref_random_pm1(int64_t n, const uint32_t *seeds, float *out, uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) { unsigned int s = seeds[k]; out[k] = random_float(s, -1.0, 1.0); out_seeds[k] = s; }
}
void ref_random_in_unit_sphere(int64_t n, const uint32_t *seeds, float *out, uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) { unsigned int s = seeds[k]; put(out + 3 * k, random_in_unit_sphere(s)); out_seeds[k] = s; }
}
void ref_random_unit_vector(int64_t n, const uint32_t *seeds, float *out, uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) { unsigned int s = seeds[k]; put(out + 3 * k, random_unit_vector(s)); out_seeds[k] = s; }
}
void ref_random_in_hemisphere(int64_t n, const uint32_t *seeds, const float *normals, float *out, uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) { unsigned int s = seeds[k]; put(out + 3 * k, random_in_hemisphere(v(normals + 3 * k), s)); out_seeds[k] = s; }
}
void ref_reflectance(int64_t n, const float *cosine, const float *ref_idx, float *out) {
    for (int64_t k = 0; k < n; ++k) out[k] = reflectance(cosine[k], ref_idx[k]);
}
// material_scatter: item k = ray k into the hit (point, normal, front_face) k on material k.  Attenuation and the scattered ray are
// written only where it returns true.
void ref_material_scatter(int64_t n, const float *ray_o, const float *ray_d, const float *point, const float *normal, const int32_t *front,
                          const PlainMaterial *mats, const uint32_t *seeds, int32_t *out_ret, float *out_att, float *out_o, float *out_d,
                          uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) {
        HitRecord rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.point = v(point + 3 * k);
        rec.normal = v(normal + 3 * k);
        rec.front_face = front[k] != 0;
        const MaterialData mat = make_material(mats[k], nullptr);
        color att(0, 0, 0);
        Ray scattered(vec3(0, 0, 0), vec3(0, 0, 0));
        unsigned int s = seeds[k];
        out_ret[k] = material_scatter(Ray(v(ray_o + 3 * k), v(ray_d + 3 * k)), rec, att, scattered, s, mat) ? 1 : 0;
        out_seeds[k] = s;
        if (out_ret[k]) { put(out_att + 3 * k, att); put(out_o + 3 * k, scattered.origin()); put(out_d + 3 * k, scattered.direction()); }
    }
}
void ref_material_emit(int64_t n, const PlainMaterial *mats, float *out) {
    for (int64_t k = 0; k < n; ++k) put(out + 3 * k, material_emit(make_material(mats[k], nullptr)));
}
// tex2D_cpu.  The caller never hands over a (u, v) at which the reference reads outside its rows (see tests/ref_shade_cases.py).
void ref_tex2d(float *rgba, int32_t width, int32_t height, int64_t n, const float *u, const float *vv, float *out) {
    CpuTexture tex{rgba, width, height};
    for (int64_t k = 0; k < n; ++k) put(out + 3 * k, tex2D_cpu(&tex, u[k], vv[k]));
}
// CameraData::get_ray: cams = n records of 76 bytes
void ref_get_ray(int64_t n, const uint8_t *cams76, const int32_t *ij, const uint32_t *seeds, float *out_o, float *out_d, uint32_t *out_seeds) {
    for (int64_t k = 0; k < n; ++k) {
        CameraData cam;
        std::memcpy(&cam, cams76 + 76 * k, 76);
        unsigned int s = seeds[k];
        const Ray r = cam.get_ray(ij[2 * k], ij[2 * k + 1], s);
        put(out_o + 3 * k, r.origin()); put(out_d + 3 * k, r.direction());
        out_seeds[k] = s;
    }
}
// Camera::build_camera_data: item k = (look-from, look-at, vfov, width, height, spp, depth, background) → 76 bytes
void ref_build_camera_data(int64_t n, const float *from, const float *at, const float *vfov, const int32_t *whsd, const float *background,
                           uint8_t *out76) {
    for (int64_t k = 0; k < n; ++k) {
        Camera cam(whsd[4 * k + 1], whsd[4 * k], nullptr, v(from + 3 * k), v(at + 3 * k));
        cam.vfov = vfov[k];
        cam.samplesPerPixel = whsd[4 * k + 2];
        cam.maxDepth = whsd[4 * k + 3];
        cam.background_color = v(background + 3 * k);
        const CameraData d = cam.build_camera_data();
        std::memcpy(out76 + 76 * k, &d, 76);
    }
}
// BinarySaver::writeColor for n sums at one spp, through the file `path` (in a temporary directory of the caller's), read back.
// Returns 0 when the file holds the 8-byte header and 3 n bytes.
int32_t ref_write_color(int64_t n, const float *sums, int32_t spp, const char *path, uint8_t *out) {
    {
        BinarySaver saver(spp, path);
        saver.setFormat((int)n, 1);
        for (int64_t k = 0; k < n; ++k) saver.writeColor(v(sums + 3 * k));
    }
    std::ifstream in(path, std::ios::binary);
    int32_t hdr[2] = {0, 0};
    in.read(reinterpret_cast<char *>(hdr), 8);
    in.read(reinterpret_cast<char *>(out), 3 * n);
    return (in && hdr[0] == (int32_t)n && hdr[1] == 1 && in.gcount() == 3 * n) ? 0 : 1;
}
int32_t ref_sizeof_camera_data(void) { return (int32_t)sizeof(CameraData); }
int32_t ref_sizeof_material_data(void) { return (int32_t)sizeof(MaterialData); }

// ray_color_host for n samples (i, j, s), each seeded as render_cpu seeds it (src/camera.cu:41-44): radiance and final seed
void ref_trace_samples(int32_t ns, const float *spheres5, int32_t np, const float *planes11, int32_t nm, const PlainMaterial *mats, int32_t nt,
                       float *tex_data, const int64_t *tex_dims, const uint8_t *cam76, int64_t n, const int32_t *ijs, float *out_rad,
                       uint32_t *out_seeds) {
    RefScene sc;
    make_scene(sc, ns, spheres5, np, planes11, nm, mats, nt, tex_data, tex_dims);
    CameraData cam;
    std::memcpy(&cam, cam76, 76);
    for (int64_t k = 0; k < n; ++k) {
        // the state render_cpu starts sample (column, row, s) from (src/camera.cu:41,43): two hashes, in 32-bit words — its size_t
        // index arithmetic is narrowed to unsigned int by wang_hash's parameter, which is the same thing
        const int column = ijs[3 * k], row = ijs[3 * k + 1];
        const uint32_t pixel_word = (uint32_t)column * (uint32_t)cam.image_width + (uint32_t)row;
        unsigned int state = wang_hash(wang_hash(pixel_word) + (uint32_t)ijs[3 * k + 2]);
        const Ray camera_ray = cam.get_ray(column, row, state);
        put(out_rad + 3 * k, ray_color_host(camera_ray, state, sc.data, cam));
        out_seeds[k] = state;
    }
}
// Camera::render_cpu of a whole (small) frame: the camera is built by the reference's own constructor + build_camera_data
void ref_render_cpu(int32_t ns, const float *spheres5, int32_t np, const float *planes11, int32_t nm, const PlainMaterial *mats, int32_t nt,
                    float *tex_data, const int64_t *tex_dims, const float *from, const float *at, float vfov, const int32_t *whsd,
                    const float *background, float *out_fb) {
    RefScene sc;
    make_scene(sc, ns, spheres5, np, planes11, nm, mats, nt, tex_data, tex_dims);
    Camera cam(whsd[1], whsd[0], nullptr, v(from), v(at));
    cam.vfov = vfov;
    cam.samplesPerPixel = whsd[2];
    cam.maxDepth = whsd[3];
    cam.background_color = v(background);
    std::vector<color> fb((size_t)whsd[0] * whsd[1]);
    cam.render_cpu(sc.data, fb);
    std::memcpy(out_fb, fb.data(), fb.size() * sizeof(color));
}

}  // extern "C"
