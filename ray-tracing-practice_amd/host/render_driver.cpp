// render_driver.cpp — the part of the host mirror that talks to the GPU library through the C ABI:
// Camera::render (src/camera.cu:198-216), gpu_render (src/camera.cu:290-349) and the
// checkCudaErrors equivalent.  Kept apart from camera.cpp so the pure-host library
// (librtp_host.so) has no dependency on librtp_amd.so.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>
#include <thread>

#include <unistd.h>

#include "camera.h"
#include "scene_params.h"

namespace rtp {

// ---- error handling ---------------------------------------------------------------------------

void check_rt(rt_status st, const char *expr, const char *file, int line) {
    if (st == RT_OK) return;
    std::cerr << "RT error = " << static_cast<unsigned>(st) << " at " << file << ":" << line << " '" << expr << "' "
              << rt_get_last_error_string() << "\n";
    std::exit(99);
}

namespace { thread_local rt_scene *g_bound_scene = nullptr; }
void bind_scene(rt_scene *scene) { g_bound_scene = scene; }
rt_scene *bound_scene() { return g_bound_scene; }

void Camera::render(float *d_fb) const {
    const size_t num_pixels = static_cast<size_t>(image_width) * image_height;
    const rt_camera_data cam = build_camera_data();  // cudaMemcpyToSymbol(d_cam_data_const), src/camera.cu:324-325
    rt_timing_init(&last_timing);
    RTP_CHECK(rt_render(bound_scene(), &cam, nullptr, d_fb, nullptr, 1, &last_timing));

    std::vector<float> host_fb(num_pixels * 3);
    RTP_CHECK(rt_copy_to_host(host_fb.data(), d_fb, num_pixels * 3 * sizeof(float)));
    if (!saver) return;
    for (size_t p = 0; p < num_pixels; ++p)
        saver->write_color(Vec3(host_fb[3 * p], host_fb[3 * p + 1], host_fb[3 * p + 2]));
}


// Frame file name.  The reference hands the pattern it read from the config straight to
// snprintf(filename, 256, pattern, n) (src/camera.cu:298-299): a pattern with anything but one integer conversion
// is undefined behaviour there.  Same result for the patterns that are defined — "%d", "%5d", "%03d", "%%", the
// 255-character truncation — and a clean failure (message + exit 99, like every other fatal error of the driver)
// for the rest, instead of passing untrusted text to printf.
std::string frame_filename(const std::string &pattern, int n) {
    std::string out;
    int conversions = 0;
    for (size_t k = 0; k < pattern.size(); ++k) {
        if (pattern[k] != '%') { out.push_back(pattern[k]); continue; }
        if (k + 1 < pattern.size() && pattern[k + 1] == '%') { out.push_back('%'); ++k; continue; }
        size_t e = k + 1;
        std::string spec = "%";
        if (e < pattern.size() && (pattern[e] == '0' || pattern[e] == '-')) spec.push_back(pattern[e++]);
        int digits = 0;
        while (e < pattern.size() && pattern[e] >= '0' && pattern[e] <= '9' && digits < 3) { spec.push_back(pattern[e++]); ++digits; }
        if (e >= pattern.size() || (pattern[e] != 'd' && pattern[e] != 'i') || ++conversions > 1) {
            std::fprintf(stderr, "output path pattern '%s': only one %%d (optionally %%0Nd / %%Nd) is supported\n", pattern.c_str());
            std::exit(99);
        }
        spec.push_back('d');
        char buf[32];
        std::snprintf(buf, sizeof(buf), spec.c_str(), n);
        out += buf;
        k = e;
    }
    if (out.size() > 255) out.resize(255);
    return out;
}

void gpu_render(const SceneParams &params, bool aov, bool denoise, bool temporal) {
    float *d_fb = nullptr;
    const size_t num_pixels = static_cast<size_t>(params.width) * params.height;
    RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_fb)));
    // --aov: the first-hit AOVs of every frame (albedo, normal, depth, hit count; rt_render_aov)
    rt_aov_buffers aov_bufs;
    rt_aov_buffers_init(&aov_bufs);
    std::vector<float> h_albedo, h_normal, h_depth;
    std::vector<uint32_t> h_hits;
    if (aov || denoise || temporal) {
        RTP_CHECK(rt_device_alloc(num_pixels * 12, reinterpret_cast<void **>(&aov_bufs.albedo_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 12, reinterpret_cast<void **>(&aov_bufs.normal_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov_bufs.depth_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov_bufs.hit_count)));
        h_albedo.resize(num_pixels * 3);
        h_normal.resize(num_pixels * 3);
        h_depth.resize(num_pixels);
        h_hits.resize(num_pixels);
    }
    // --denoise-temporal: first_prim as well, and two history buffers swapped after every frame
    void *d_history[2] = {nullptr, nullptr};
    const uint64_t history_bytes = temporal ? rt_denoise_history_bytes(params.width, params.height) : 0;
    if (temporal) {
        RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov_bufs.first_prim)));
        RTP_CHECK(rt_device_alloc(history_bytes, &d_history[0]));
        RTP_CHECK(rt_device_alloc(history_bytes, &d_history[1]));
    }
    // --denoise / --denoise-temporal: the filter's workspace and output (the sum over samples, like d_fb)
    void *d_workspace = nullptr;
    float *d_denoised = nullptr;
    const uint64_t workspace_bytes = denoise || temporal ? rt_denoise_workspace_bytes(params.width, params.height) : 0;
    std::vector<float> h_denoised;
    if (denoise || temporal) {
        RTP_CHECK(rt_device_alloc(workspace_bytes, &d_workspace));
        RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_denoised)));
        h_denoised.resize(num_pixels * 3);
    }

    for (int n = 0; n < params.num_frames; ++n) {
        const std::string filename = frame_filename(params.output_pattern, n);
        auto saver = std::make_unique<BinarySaver>(params.sqrt_spp, filename);
        Vec3 eye, target;
        orbit_pose(params, n, eye, target);

        Camera camera(params.height, params.width, std::move(saver), eye, target);
        camera.vfov = params.fov_degrees;
        camera.samples_per_pixel = params.sqrt_spp * params.sqrt_spp;
        camera.max_depth = params.max_depth;
        camera.background_color = Vec3(0, 0, 0);

        // the reference brackets Camera::render — kernel, D2H and saver I/O — with events
        const auto t0 = std::chrono::steady_clock::now();
        camera.render(d_fb);
        const auto t1 = std::chrono::steady_clock::now();
        const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
        const long long total_rays = static_cast<long long>(params.width) * params.height * params.sqrt_spp * params.sqrt_spp;
        std::cout << n << "\t" << ms << "\t" << total_rays << "\n";
        if (aov || denoise || temporal) {          // (outside the frame's timed span: the reference has no such output)
            const rt_camera_data cam = camera.build_camera_data();
            RTP_CHECK(rt_render_aov(bound_scene(), &cam, nullptr, &aov_bufs, nullptr, 1, nullptr));
            if (aov) {
                RTP_CHECK(rt_copy_to_host(h_albedo.data(), aov_bufs.albedo_sum, num_pixels * 12));
                RTP_CHECK(rt_copy_to_host(h_normal.data(), aov_bufs.normal_sum, num_pixels * 12));
                RTP_CHECK(rt_copy_to_host(h_depth.data(), aov_bufs.depth_sum, num_pixels * 4));
                RTP_CHECK(rt_copy_to_host(h_hits.data(), aov_bufs.hit_count, num_pixels * 4));
                if (!write_aov_file(filename + ".aov", params.width, params.height, cam.samples_per_pixel, h_albedo.data(), h_normal.data(),
                                    h_depth.data(), h_hits.data())) {
                    std::cerr << "cannot write " << filename << ".aov\n";
                    std::exit(99);
                }
            }
            if (denoise || temporal) {       // the frame's own saver code and divisor, into "<frame file>.denoised"
                if (denoise)
                    RTP_CHECK(rt_denoise(d_fb, &aov_bufs, params.width, params.height, cam.samples_per_pixel, nullptr, d_workspace, workspace_bytes,
                                         d_denoised, nullptr));
                else       // frame n reads the history frame n - 1 wrote (frame 0: none)
                    RTP_CHECK(rt_denoise_temporal(d_fb, &aov_bufs, &cam, nullptr, n == 0 ? nullptr : d_history[(n + 1) & 1], d_history[n & 1],
                                                  history_bytes, d_workspace, workspace_bytes, d_denoised, nullptr));
                RTP_CHECK(rt_copy_to_host(h_denoised.data(), d_denoised, num_pixels * 3 * sizeof(float)));
                BinarySaver out(params.sqrt_spp, filename + ".denoised");
                out.set_format(params.width, params.height);
                for (size_t p = 0; p < num_pixels; ++p) out.write_color(Vec3(h_denoised[3 * p], h_denoised[3 * p + 1], h_denoised[3 * p + 2]));
            }
        }
    }
    rt_device_free(d_fb);  // unchecked in the reference too (src/camera.cu:348)
    rt_device_free(aov_bufs.albedo_sum);
    rt_device_free(aov_bufs.normal_sum);
    rt_device_free(aov_bufs.depth_sum);
    rt_device_free(aov_bufs.hit_count);
    rt_device_free(aov_bufs.first_prim);
    rt_device_free(d_history[0]);
    rt_device_free(d_history[1]);
    rt_device_free(d_workspace);
    rt_device_free(d_denoised);
}

// ---- animation driver ("next" rows f1 + f2 of SURVEY.md §8) ---------------------------------------
// The reference renders its frames one after the other on one GPU and spends most of each frame's
// wall time pushing pixels through three 1-byte ofstream writes (src/camera.cu:211-215,148-152).
// Frames are independent (each has its own camera pose and output file), so here
//   * frames are dealt round-robin to `num_devices` GPUs, one host thread and one rt_scene per GPU;
//   * the saver arithmetic runs on the device (rt_tonemap: byte-exact ISaver::writeColor), so
//     the D2H copy is RGB8 (4x smaller than the float sums);
//   * the file of frame n is written by a writer thread while frame n+1 renders.
// The files are byte-identical to what gpu_render() above (and the reference) writes.
namespace {

struct PendingFile {
    std::string path;
    int width = 0, height = 0;
    std::vector<uint8_t> rgb;
};

void write_binary_frame(const PendingFile &f) {
    std::ofstream out(f.path, std::ios::binary);
    const int32_t hdr[2] = {f.width, f.height};     // BinarySaver::setFormat (src/camera.cu:131-136)
    out.write(reinterpret_cast<const char *>(hdr), sizeof(hdr));
    out.write(reinterpret_cast<const char *>(f.rgb.data()), static_cast<std::streamsize>(f.rgb.size()));
}

// rtp_main --denoise-adaptive: what both adaptive drivers keep for it — the frame's moments, AOVs at min_spp, rt_denoise's workspace
// and the filtered frame — and the step after a frame's AOVs are rendered: rt_denoise_spp, rt_tonemap_spp, "<frame file>.denoised".
// temporal (rtp_main --denoise-adaptive-temporal): first_prim as well and two history buffers swapped after every
// frame, and the step is rt_denoise_temporal_spp with the frame's camera
struct AdaptiveDenoiser {
    int width = 0, height = 0;
    size_t num_pixels = 0;
    float *d_moments = nullptr, *d_denoised = nullptr;
    void *d_workspace = nullptr;
    uint64_t workspace_bytes = 0;
    rt_aov_buffers aov;
    bool temporal = false;
    void *d_history[2] = {nullptr, nullptr};
    uint64_t history_bytes = 0;
    int frames = 0;
    float *d_prior = nullptr;          // rtp_main --stop-history: the prior of the frame about to be rendered

    AdaptiveDenoiser(int w, int h, bool temporal_ = false, bool stop_history = false)
        : width(w), height(h), num_pixels(static_cast<size_t>(w) * h), temporal(temporal_) {
        rt_aov_buffers_init(&aov);
        workspace_bytes = rt_denoise_workspace_bytes(w, h);
        RTP_CHECK(rt_device_alloc(num_pixels * 8, reinterpret_cast<void **>(&d_moments)));
        RTP_CHECK(rt_device_alloc(num_pixels * 12, reinterpret_cast<void **>(&d_denoised)));
        RTP_CHECK(rt_device_alloc(workspace_bytes, &d_workspace));
        RTP_CHECK(rt_device_alloc(num_pixels * 12, reinterpret_cast<void **>(&aov.albedo_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 12, reinterpret_cast<void **>(&aov.normal_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov.depth_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov.hit_count)));
        if (temporal) {
            history_bytes = rt_denoise_history_bytes(w, h);
            RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov.first_prim)));
            RTP_CHECK(rt_device_alloc(history_bytes, &d_history[0]));
            RTP_CHECK(rt_device_alloc(history_bytes, &d_history[1]));
            if (stop_history) RTP_CHECK(rt_device_alloc(num_pixels * 8, reinterpret_cast<void **>(&d_prior)));
        }
    }
    ~AdaptiveDenoiser() {
        rt_device_free(aov.first_prim);
        rt_device_free(d_prior);
        rt_device_free(d_history[0]);
        rt_device_free(d_history[1]);
        rt_device_free(d_moments);
        rt_device_free(d_denoised);
        rt_device_free(d_workspace);
        rt_device_free(aov.albedo_sum);
        rt_device_free(aov.normal_sum);
        rt_device_free(aov.depth_sum);
        rt_device_free(aov.hit_count);
    }
    AdaptiveDenoiser(const AdaptiveDenoiser &) = delete;
    AdaptiveDenoiser &operator=(const AdaptiveDenoiser &) = delete;

    // With the frame's AOVs at aov_samples in place: the prior from the history the frame's write() will read (none on the first frame)
    void make_prior(int32_t aov_samples, const rt_camera_data &cam) {
        RTP_CHECK(rt_adaptive_prior(&aov, aov_samples, &cam, frames == 0 ? nullptr : d_history[(frames + 1) & 1], history_bytes, d_prior, nullptr));
    }

    // d_rgb: the frame's own byte buffer, free again once the frame's file is written
    // cam: the frame's camera (the temporal filter's reprojection; unused without it)
    void write(const std::string &filename, const float *d_fb, const int32_t *d_spp, int32_t aov_samples, uint8_t *d_rgb, const rt_camera_data &cam) {
        if (temporal) {
            RTP_CHECK(rt_denoise_temporal_spp(d_fb, d_spp, d_moments, &aov, aov_samples, &cam, nullptr, frames == 0 ? nullptr : d_history[(frames + 1) & 1],
                                              d_history[frames & 1], history_bytes, d_workspace, workspace_bytes, d_denoised, nullptr));
            ++frames;
        } else {
            RTP_CHECK(rt_denoise_spp(d_fb, d_spp, d_moments, &aov, aov_samples, width, height, nullptr, d_workspace, workspace_bytes, d_denoised, nullptr));
        }
        RTP_CHECK(rt_tonemap_spp(d_denoised, d_spp, d_rgb, static_cast<int64_t>(num_pixels), nullptr));
        PendingFile file;
        file.path = filename + ".denoised";
        file.width = width;
        file.height = height;
        file.rgb.resize(num_pixels * 3);
        RTP_CHECK(rt_copy_to_host(file.rgb.data(), d_rgb, num_pixels * 3));
        write_binary_frame(file);
    }
};

}  // namespace

void gpu_render_pipelined(const SceneParams &params, const rt_scene_desc &desc, int num_devices) {
    if (num_devices < 1) num_devices = 1;
    std::mutex print_mutex;
    auto worker = [&](int dev) {
        RTP_CHECK(rt_set_device(dev));
        rt_scene *scene = nullptr;
        RTP_CHECK(rt_scene_create(&desc, &scene));
        const size_t num_pixels = static_cast<size_t>(params.width) * params.height;
        float *d_fb = nullptr;
        uint8_t *d_rgb = nullptr;
        RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_fb)));
        RTP_CHECK(rt_device_alloc(num_pixels * 3, reinterpret_cast<void **>(&d_rgb)));
        std::thread writer;
        for (int n = dev; n < params.num_frames; n += num_devices) {
            const std::string filename = frame_filename(params.output_pattern, n);
            Vec3 eye, target;
            orbit_pose(params, n, eye, target);
            Camera camera(params.height, params.width, nullptr, eye, target);
            camera.vfov = params.fov_degrees;
            camera.samples_per_pixel = params.sqrt_spp * params.sqrt_spp;
            camera.max_depth = params.max_depth;
            camera.background_color = Vec3(0, 0, 0);
            const rt_camera_data cam = camera.build_camera_data();

            const auto t0 = std::chrono::steady_clock::now();
            rt_timing timing;
            rt_timing_init(&timing);
            RTP_CHECK(rt_render(scene, &cam, nullptr, d_fb, nullptr, 1, &timing));
            RTP_CHECK(rt_tonemap(d_fb, d_rgb, static_cast<int64_t>(num_pixels) * 3, params.sqrt_spp, nullptr));
            auto file = std::make_shared<PendingFile>();
            file->path = filename;
            file->width = params.width;
            file->height = params.height;
            file->rgb.resize(num_pixels * 3);
            RTP_CHECK(rt_copy_to_host(file->rgb.data(), d_rgb, num_pixels * 3));
            if (writer.joinable()) writer.join();           // at most one file in flight per GPU
            writer = std::thread([file]() { write_binary_frame(*file); });
            const auto t1 = std::chrono::steady_clock::now();
            const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
            const long long total_rays = static_cast<long long>(params.width) * params.height * params.sqrt_spp * params.sqrt_spp;
            std::lock_guard<std::mutex> lock(print_mutex);
            std::cout << n << "\t" << ms << "\t" << total_rays << "\n";
        }
        if (writer.joinable()) writer.join();
        rt_device_free(d_fb);
        rt_device_free(d_rgb);
        RTP_CHECK(rt_scene_destroy(scene));
    };
    std::vector<std::thread> threads;
    for (int d = 1; d < num_devices; ++d) threads.emplace_back(worker, d);
    worker(0);
    for (std::thread &t : threads) t.join();
}

// ---- thin lens and open shutter (rtp_main --gpu --lens R:F --motion-blur S) ---------------------------------------
// The orbit of gpu_render, each frame through rt_render_lens: the shutter opens at frame n and closes at n + shutter (0: no motion),
// the lens has radius lens.lens_radius.  Saved through rt_tonemap with the frame's divisor — the bytes gpu_render's saver writes for
// these sums.  aov / denoise as in gpu_render, from rt_render_aov_lens.
// nee: the frames through rt_render_nee (rtp_main --nee), the AOVs through rt_render_aov_samples — the same first hits; env: through
// rt_render_env with env_params (rtp_main --env), the AOVs likewise; lit: through rt_render_lit (rtp_main --lit) with this lens and
// shutter, the AOVs through rt_render_aov_lens; noise (with lit; rtp_main --lit --noise-target): through
// rt_render_lit_adaptive and rt_tonemap_spp — every pixel's bytes at its own sample count — and the printed count is the samples taken
// medium (with lit, without noise; rtp_main --lit --fog): through rt_render_medium; volume (with medium; rtp_main --fog-grid,
// DESIGN.md §28): through rt_render_volume with this grid in the medium's box.  medium with noise (rtp_main --fog-noise-target, DESIGN.md
// §29): through rt_render_volume_adaptive (the volume may be null) and rt_tonemap_spp, without a stop rule or a prior.  medium with
// fog_adaptive (rtp_main --fog-adaptive): the same through rt_render_fog_adaptive, under chroma, glow and glow_sample too.
// fog_denoise (with medium; rtp_main --fog-denoise): denoise — or with noise denoise_adaptive — with the AOVs from
// rt_render_aov_volume under the frame's own lit, medium and volume.
// denoise_adaptive (with noise; rtp_main --denoise-adaptive): as in gpu_render_adaptive, the AOVs from rt_render_aov_lens at noise->min_spp
void gpu_render_lens(const SceneParams &params, const rt_scene_desc &desc, const FrameJob &job) {
    rt_lens_params pinhole;
    rt_lens_params_init(&pinhole);
    const rt_lens_params &lens = job.lens ? *job.lens : pinhole;
    const float shutter = job.shutter;
    const bool aov = job.aov, fog_denoise = job.fog_denoise, denoise_adaptive_temporal = job.denoise_adaptive_temporal;
    const rt_nee_params *nee = job.nee;
    const rt_env *env = job.env;
    const rt_lit_params *lit = job.lit;
    // the adaptive parameters of the job's frames, whichever flag gave them (the counts, rt_tonemap_spp and the denoisers read these)
    const rt_adaptive_params *noise = job.fog_adaptive ? job.fog_adaptive : job.noise;
    const rt_medium_params *medium = job.medium;
    const rt_volume *volume = job.volume;
    const bool denoise = job.denoise || (fog_denoise && !noise), denoise_adaptive = job.denoise_adaptive || (fog_denoise && noise);
    rt_scene *scene = nullptr;
    RTP_CHECK(rt_scene_create(&desc, &scene));
    const size_t num_pixels = static_cast<size_t>(params.width) * params.height;
    float *d_fb = nullptr, *d_denoised = nullptr;
    uint8_t *d_rgb = nullptr;
    void *d_workspace = nullptr;
    const bool split = job.split && lit && !noise && !medium;
    const uint64_t workspace_bytes = !denoise ? 0 : split ? rt_denoise_split_workspace_bytes(params.width, params.height) : rt_denoise_workspace_bytes(params.width, params.height);
    RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_fb)));
    RTP_CHECK(rt_device_alloc(num_pixels * 3, reinterpret_cast<void **>(&d_rgb)));
    // --split: the two components on the device, and on the host for their files and their sum
    float *d_direct = nullptr, *d_indirect = nullptr;
    std::vector<float> h_direct, h_indirect;
    if (split) {
        RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_direct)));
        RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_indirect)));
        h_direct.resize(num_pixels * 3);
        h_indirect.resize(num_pixels * 3);
    }
    auto save_sums = [&](const std::string &path, const float *sums) {          // the frame's own saver code and divisor
        BinarySaver out(params.sqrt_spp, path);
        out.set_format(params.width, params.height);
        for (size_t p = 0; p < num_pixels; ++p) out.write_color(Vec3(sums[3 * p], sums[3 * p + 1], sums[3 * p + 2]));
    };
    int32_t *d_spp = nullptr;
    std::vector<int32_t> h_spp;
    if (lit && noise) {
        RTP_CHECK(rt_device_alloc(num_pixels * sizeof(int32_t), reinterpret_cast<void **>(&d_spp)));
        h_spp.resize(num_pixels);
    }
    std::unique_ptr<AdaptiveDenoiser> spp_denoiser;
    if (lit && noise && (denoise_adaptive || denoise_adaptive_temporal))
        spp_denoiser = std::make_unique<AdaptiveDenoiser>(params.width, params.height, denoise_adaptive_temporal, job.stop_history);
    const bool with_prior = spp_denoiser && spp_denoiser->d_prior;
    rt_aov_buffers aov_bufs;
    rt_aov_buffers_init(&aov_bufs);
    std::vector<float> h_albedo, h_normal, h_depth, h_denoised;
    std::vector<uint32_t> h_hits;
    if (aov || denoise) {
        RTP_CHECK(rt_device_alloc(num_pixels * 12, reinterpret_cast<void **>(&aov_bufs.albedo_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 12, reinterpret_cast<void **>(&aov_bufs.normal_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov_bufs.depth_sum)));
        RTP_CHECK(rt_device_alloc(num_pixels * 4, reinterpret_cast<void **>(&aov_bufs.hit_count)));
    }
    if (denoise) {
        RTP_CHECK(rt_device_alloc(workspace_bytes, &d_workspace));
        RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_denoised)));
        h_denoised.resize(num_pixels * 3);
    }
    auto camera_at = [&](float t) {
        Vec3 eye, target;
        orbit_pose_at(params, t, eye, target);
        Camera camera(params.height, params.width, nullptr, eye, target);
        camera.vfov = params.fov_degrees;
        camera.samples_per_pixel = params.sqrt_spp * params.sqrt_spp;
        camera.max_depth = params.max_depth;
        camera.background_color = Vec3(0, 0, 0);
        return camera.build_camera_data();
    };
    auto frame_lit = [&](const rt_camera_data *cam_close) {          // the job's lit call with this frame's lens and closing camera
        rt_lit_params l = *lit;
        l.cam_close = cam_close;
        l.lens = &lens;
        return l;
    };
    PendingFile file;
    file.width = params.width;
    file.height = params.height;
    file.rgb.resize(num_pixels * 3);
    for (int n = 0; n < params.num_frames; ++n) {
        const std::string filename = frame_filename(params.output_pattern, n);
        const rt_camera_data cam = camera_at(static_cast<float>(n));
        const rt_camera_data close = camera_at(static_cast<float>(n) + shutter);
        const rt_camera_data *cam_close = shutter > 0.0f ? &close : nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        long long total_rays = static_cast<long long>(params.width) * params.height * params.sqrt_spp * params.sqrt_spp;
        if (lit && noise && with_prior) {          // (a pinhole, no shutter) the first hits at min_spp, the prior, the frame
            const rt_lit_params lit_now = frame_lit(cam_close);
            rt_camera_data aov_cam = cam;
            aov_cam.samples_per_pixel = noise->min_spp;
            RTP_CHECK(rt_render_aov(scene, &aov_cam, nullptr, &spp_denoiser->aov, nullptr, 1, nullptr));
            spp_denoiser->make_prior(noise->min_spp, cam);
            RTP_CHECK(rt_render_lit_adaptive_prior(scene, &cam, &lit_now, noise, job.stop, nullptr, 0, d_fb, d_spp, spp_denoiser->d_moments, nullptr, 1, nullptr,
                                                   spp_denoiser->d_prior));
        } else if (lit && noise) {
            const rt_lit_params lit_now = frame_lit(cam_close);
            if (medium && job.fog_adaptive) {          // (rtp_main --fog-adaptive: the rung by the job's members; no stop rule, no prior)
                rt_fog_params fog;
                rt_fog_params_init(&fog);
                fog.medium = medium;
                fog.volume = volume;
                fog.chroma = job.chroma;
                fog.glow = job.glow;
                fog.heat = job.heat;
                fog.sample = job.glow ? job.glow_sample : nullptr;
                fog.sampler = job.sampler;
                RTP_CHECK(rt_render_fog_adaptive(scene, &cam, &lit_now, &fog, noise, nullptr, nullptr, nullptr, 0, d_fb, d_spp, nullptr, nullptr, 1, nullptr));
            } else if (medium)          // (rtp_main --fog-noise-target: no stop rule, no prior; the moments for --fog-denoise)
                RTP_CHECK(rt_render_volume_adaptive(scene, &cam, &lit_now, medium, volume, noise, nullptr, nullptr, nullptr, 0, d_fb, d_spp,
                                                    spp_denoiser ? spp_denoiser->d_moments : nullptr, nullptr, 1, nullptr));
            else
                RTP_CHECK(rt_render_lit_adaptive_rule(scene, &cam, &lit_now, noise, job.stop, nullptr, 0, d_fb, d_spp,
                                                      spp_denoiser ? spp_denoiser->d_moments : nullptr, nullptr, 1, nullptr));
        } else if (split) {
            const rt_lit_params lit_now = frame_lit(cam_close);
            RTP_CHECK(rt_render_lit_split(scene, &cam, &lit_now, nullptr, 0, d_direct, d_indirect, nullptr, 1, nullptr));
        } else if (lit) {
            const rt_lit_params lit_now = frame_lit(cam_close);
            if (medium && job.chroma) RTP_CHECK(rt_render_chroma(scene, &cam, &lit_now, medium, volume, job.chroma, nullptr, 0, d_fb, nullptr, 1, nullptr));
            else if (medium && job.glow && job.glow_sample)
                RTP_CHECK(rt_render_glow_sampled(scene, &cam, &lit_now, medium, volume, job.glow, job.heat, job.glow_sample, job.sampler, nullptr, 0, d_fb, nullptr, 1, nullptr));
            else if (medium && job.glow) RTP_CHECK(rt_render_glow(scene, &cam, &lit_now, medium, volume, job.glow, job.heat, nullptr, 0, d_fb, nullptr, 1, nullptr));
            else if (medium && volume) RTP_CHECK(rt_render_volume(scene, &cam, &lit_now, medium, volume, nullptr, 0, d_fb, nullptr, 1, nullptr));
            else if (medium) RTP_CHECK(rt_render_medium(scene, &cam, &lit_now, medium, nullptr, 0, d_fb, nullptr, 1, nullptr));
            else RTP_CHECK(rt_render_lit(scene, &cam, &lit_now, nullptr, 0, d_fb, nullptr, 1, nullptr));
        } else if (env) RTP_CHECK(rt_render_env(scene, &cam, env, job.env_params, nullptr, 0, d_fb, nullptr, 1, nullptr));
        else if (nee) RTP_CHECK(rt_render_nee(scene, &cam, nee, nullptr, 0, d_fb, nullptr, 1, nullptr));
        else RTP_CHECK(rt_render_lens(scene, &cam, cam_close, &lens, nullptr, 0, d_fb, nullptr, 1, nullptr));
        if (split) {          // the components' files; the frame from their sum, one float32 add per channel
            RTP_CHECK(rt_copy_to_host(h_direct.data(), d_direct, num_pixels * 3 * sizeof(float)));
            RTP_CHECK(rt_copy_to_host(h_indirect.data(), d_indirect, num_pixels * 3 * sizeof(float)));
            save_sums(filename + ".direct", h_direct.data());
            save_sums(filename + ".indirect", h_indirect.data());
            for (size_t k = 0; k < num_pixels * 3; ++k) h_direct[k] = h_direct[k] + h_indirect[k];
            save_sums(filename, h_direct.data());
        } else if (d_spp) {
            RTP_CHECK(rt_tonemap_spp(d_fb, d_spp, d_rgb, static_cast<int64_t>(num_pixels), nullptr));
            RTP_CHECK(rt_copy_to_host(h_spp.data(), d_spp, num_pixels * sizeof(int32_t)));
            total_rays = 0;
            for (int32_t k : h_spp) total_rays += k;
        } else {
            RTP_CHECK(rt_tonemap(d_fb, d_rgb, static_cast<int64_t>(num_pixels) * 3, params.sqrt_spp, nullptr));
        }
        if (!split) {
            RTP_CHECK(rt_copy_to_host(file.rgb.data(), d_rgb, num_pixels * 3));
            file.path = filename;
            write_binary_frame(file);
        }
        const auto t1 = std::chrono::steady_clock::now();
        const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
        std::cout << n << "\t" << ms << "\t" << total_rays << "\n";
        if (spp_denoiser) {          // (outside the frame's timed span) the first hits of this lens and shutter at min_spp samples
            rt_camera_data aov_open = cam, aov_close = close;
            aov_open.samples_per_pixel = aov_close.samples_per_pixel = noise->min_spp;
            if (with_prior) {          // (rendered before the frame)
            } else if (fog_denoise) {
                const rt_lit_params lit_now = frame_lit(cam_close ? &aov_close : nullptr);
                RTP_CHECK(rt_render_aov_volume(scene, &aov_open, &lit_now, medium, volume, nullptr, 0, &spp_denoiser->aov, nullptr, nullptr, 1, nullptr));
            } else if (spp_denoiser->temporal) {
                RTP_CHECK(rt_render_aov(scene, &aov_open, nullptr, &spp_denoiser->aov, nullptr, 1, nullptr));       // (a pinhole, no shutter)
            } else {
                RTP_CHECK(rt_render_aov_lens(scene, &aov_open, cam_close ? &aov_close : nullptr, &lens, nullptr, 0, &spp_denoiser->aov, nullptr, 1, nullptr));
            }
            spp_denoiser->write(filename, d_fb, d_spp, noise->min_spp, d_rgb, cam);
        }
        if (aov || denoise) {          // (outside the frame's timed span, as in gpu_render)
            if (!lit && (nee || env)) RTP_CHECK(rt_render_aov_samples(scene, &cam, nullptr, 0, &aov_bufs, nullptr, 1, nullptr));
            else if (fog_denoise) {
                const rt_lit_params lit_now = frame_lit(cam_close);
                RTP_CHECK(rt_render_aov_volume(scene, &cam, &lit_now, medium, volume, nullptr, 0, &aov_bufs, nullptr, nullptr, 1, nullptr));
            } else RTP_CHECK(rt_render_aov_lens(scene, &cam, cam_close, &lens, nullptr, 0, &aov_bufs, nullptr, 1, nullptr));
            if (aov) {
                h_albedo.resize(num_pixels * 3); h_normal.resize(num_pixels * 3); h_depth.resize(num_pixels); h_hits.resize(num_pixels);
                RTP_CHECK(rt_copy_to_host(h_albedo.data(), aov_bufs.albedo_sum, num_pixels * 12));
                RTP_CHECK(rt_copy_to_host(h_normal.data(), aov_bufs.normal_sum, num_pixels * 12));
                RTP_CHECK(rt_copy_to_host(h_depth.data(), aov_bufs.depth_sum, num_pixels * 4));
                RTP_CHECK(rt_copy_to_host(h_hits.data(), aov_bufs.hit_count, num_pixels * 4));
                if (!write_aov_file(filename + ".aov", params.width, params.height, cam.samples_per_pixel, h_albedo.data(), h_normal.data(),
                                    h_depth.data(), h_hits.data())) {
                    std::cerr << "cannot write " << filename << ".aov\n";
                    std::exit(99);
                }
            }
            if (denoise) {
                if (split)
                    RTP_CHECK(rt_denoise_split(d_direct, d_indirect, &aov_bufs, params.width, params.height, cam.samples_per_pixel, nullptr, d_workspace,
                                               workspace_bytes, d_denoised, nullptr));
                else
                    RTP_CHECK(rt_denoise(d_fb, &aov_bufs, params.width, params.height, cam.samples_per_pixel, nullptr, d_workspace, workspace_bytes,
                                         d_denoised, nullptr));
                RTP_CHECK(rt_copy_to_host(h_denoised.data(), d_denoised, num_pixels * 3 * sizeof(float)));
                BinarySaver out(params.sqrt_spp, filename + ".denoised");
                out.set_format(params.width, params.height);
                for (size_t p = 0; p < num_pixels; ++p) out.write_color(Vec3(h_denoised[3 * p], h_denoised[3 * p + 1], h_denoised[3 * p + 2]));
            }
        }
    }
    rt_device_free(d_direct);
    rt_device_free(d_indirect);
    rt_device_free(d_fb);
    rt_device_free(d_rgb);
    rt_device_free(d_spp);
    rt_device_free(aov_bufs.albedo_sum);
    rt_device_free(aov_bufs.normal_sum);
    rt_device_free(aov_bufs.depth_sum);
    rt_device_free(aov_bufs.hit_count);
    rt_device_free(d_workspace);
    rt_device_free(d_denoised);
    RTP_CHECK(rt_scene_destroy(scene));
}

// ---- adaptive sampling (rtp_main --gpu --adaptive) ----------------------------------------------------------
// The orbit of gpu_render, each frame rendered by rt_render_adaptive and saved through rt_tonemap_spp: every pixel's bytes are the
// saver arithmetic with its own sample count as the divisor (the mean of its samples).  Prints frame, milliseconds and the samples
// the frame took.  denoise_adaptive (rtp_main --denoise-adaptive): the frame's moments are kept, its AOVs rendered at
// min_spp, and rt_denoise_spp's output goes through rt_tonemap_spp to "<frame file>.denoised".  denoise_adaptive_temporal (rtp_main
// --denoise-adaptive-temporal): the same with rt_denoise_temporal_spp and its history from the frame before.
void gpu_render_adaptive(const SceneParams &params, const rt_scene_desc &desc, const FrameJob &job) {
    const rt_adaptive_params &ap = *job.noise;
    const rt_stop_params *stop = job.stop;
    rt_scene *scene = nullptr;
    RTP_CHECK(rt_scene_create(&desc, &scene));
    const size_t num_pixels = static_cast<size_t>(params.width) * params.height;
    float *d_fb = nullptr;
    int32_t *d_spp = nullptr;
    uint8_t *d_rgb = nullptr;
    RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_fb)));
    RTP_CHECK(rt_device_alloc(num_pixels * sizeof(int32_t), reinterpret_cast<void **>(&d_spp)));
    RTP_CHECK(rt_device_alloc(num_pixels * 3, reinterpret_cast<void **>(&d_rgb)));
    std::vector<int32_t> spp(num_pixels);
    std::unique_ptr<AdaptiveDenoiser> spp_denoiser;
    if (job.denoise_adaptive || job.denoise_adaptive_temporal)
        spp_denoiser = std::make_unique<AdaptiveDenoiser>(params.width, params.height, job.denoise_adaptive_temporal, job.stop_history);
    const bool with_prior = spp_denoiser && spp_denoiser->d_prior;
    for (int n = 0; n < params.num_frames; ++n) {
        Vec3 eye, target;
        orbit_pose(params, n, eye, target);
        Camera camera(params.height, params.width, nullptr, eye, target);
        camera.vfov = params.fov_degrees;
        camera.samples_per_pixel = ap.min_spp;
        camera.max_depth = params.max_depth;
        camera.background_color = Vec3(0, 0, 0);
        const rt_camera_data cam = camera.build_camera_data();
        const auto t0 = std::chrono::steady_clock::now();
        if (with_prior) {          // cam carries min_spp: the first hits, the prior from the frame before, the frame
            RTP_CHECK(rt_render_aov(scene, &cam, nullptr, &spp_denoiser->aov, nullptr, 1, nullptr));
            spp_denoiser->make_prior(ap.min_spp, cam);
            RTP_CHECK(rt_render_adaptive_prior(scene, &cam, nullptr, &ap, stop, d_fb, d_spp, spp_denoiser->d_moments, nullptr, 1, nullptr, spp_denoiser->d_prior));
        } else {
            RTP_CHECK(rt_render_adaptive_rule(scene, &cam, nullptr, &ap, stop, d_fb, d_spp, spp_denoiser ? spp_denoiser->d_moments : nullptr, nullptr, 1, nullptr));
        }
        RTP_CHECK(rt_tonemap_spp(d_fb, d_spp, d_rgb, static_cast<int64_t>(num_pixels), nullptr));
        PendingFile file;
        file.path = frame_filename(params.output_pattern, n);
        file.width = params.width;
        file.height = params.height;
        file.rgb.resize(num_pixels * 3);
        RTP_CHECK(rt_copy_to_host(file.rgb.data(), d_rgb, num_pixels * 3));
        RTP_CHECK(rt_copy_to_host(spp.data(), d_spp, num_pixels * sizeof(int32_t)));
        write_binary_frame(file);
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        long long samples = 0;
        for (int32_t k : spp) samples += k;
        std::cout << n << "\t" << ms << "\t" << samples << "\n";
        if (spp_denoiser) {          // (outside the frame's timed span) cam carries min_spp: the AOVs of the frame's first samples
            if (!with_prior) RTP_CHECK(rt_render_aov(scene, &cam, nullptr, &spp_denoiser->aov, nullptr, 1, nullptr));
            spp_denoiser->write(file.path, d_fb, d_spp, ap.min_spp, d_rgb, cam);
        }
    }
    spp_denoiser.reset();
    rt_device_free(d_fb);
    rt_device_free(d_spp);
    rt_device_free(d_rgb);
    RTP_CHECK(rt_scene_destroy(scene));
}

// ---- one frame over all GPUs (BASELINE configs[3]) ------------------------------------------
// The other way to use a node: every frame is split into interleaved 8-row bands over `num_devices` GPUs
// (rt_context / rt_render_sharded: scene replicated, one RCCL gather per frame to the root GPU), then the root runs
// the saver arithmetic on the device and the file is written while the next frame renders.  Same files, byte for byte.
void gpu_render_sharded(const SceneParams &params, const rt_scene_desc &desc, int num_devices) {
    rt_context *ctx = nullptr;
    {
        // RCCL prints a version banner on stdout when the first communicator is made; stdout is this program's data channel
        // (the per-frame TSV, src/camera.cu:346).  No other thread of this process exists yet, so fd 1 can point at fd 2 for
        // the duration of the call — the application's business, not the library's.
        std::cout.flush();
        fflush(stdout);
        const int saved_stdout = dup(1);
        if (saved_stdout >= 0) (void)dup2(2, 1);
        const rt_status st = rt_context_create(num_devices, nullptr, &ctx);
        fflush(stdout);
        if (saved_stdout >= 0) { (void)dup2(saved_stdout, 1); (void)close(saved_stdout); }
        RTP_CHECK(st);
    }
    RTP_CHECK(rt_context_scene_create(ctx, &desc, nullptr));
    const int n = rt_context_num_devices(ctx);
    const size_t num_pixels = static_cast<size_t>(params.width) * params.height;
    float *d_fb = nullptr;
    uint8_t *d_rgb = nullptr;
    RTP_CHECK(rt_set_device(0));
    RTP_CHECK(rt_device_alloc(num_pixels * 3 * sizeof(float), reinterpret_cast<void **>(&d_fb)));
    RTP_CHECK(rt_device_alloc(num_pixels * 3, reinterpret_cast<void **>(&d_rgb)));
    std::thread writer;
    std::vector<rt_timing> timings(static_cast<size_t>(n));
    for (rt_timing &t : timings) rt_timing_init(&t);
    for (int f = 0; f < params.num_frames; ++f) {
        const std::string filename = frame_filename(params.output_pattern, f);
        Vec3 eye, target;
        orbit_pose(params, f, eye, target);
        Camera camera(params.height, params.width, nullptr, eye, target);
        camera.vfov = params.fov_degrees;
        camera.samples_per_pixel = params.sqrt_spp * params.sqrt_spp;
        camera.max_depth = params.max_depth;
        camera.background_color = Vec3(0, 0, 0);
        const rt_camera_data cam = camera.build_camera_data();
        const auto t0 = std::chrono::steady_clock::now();
        RTP_CHECK(rt_render_sharded(ctx, &cam, 8, d_fb, timings.data()));
        RTP_CHECK(rt_tonemap(d_fb, d_rgb, static_cast<int64_t>(num_pixels) * 3, params.sqrt_spp, nullptr));
        auto file = std::make_shared<PendingFile>();
        file->path = filename;
        file->width = params.width;
        file->height = params.height;
        file->rgb.resize(num_pixels * 3);
        RTP_CHECK(rt_copy_to_host(file->rgb.data(), d_rgb, num_pixels * 3));
        if (writer.joinable()) writer.join();
        writer = std::thread([file]() { write_binary_frame(*file); });
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const long long total_rays = static_cast<long long>(params.width) * params.height * params.sqrt_spp * params.sqrt_spp;
        std::cout << f << "\t" << ms << "\t" << total_rays << "\n";
    }
    if (writer.joinable()) writer.join();
    rt_device_free(d_fb);
    rt_device_free(d_rgb);
    RTP_CHECK(rt_context_destroy(ctx));
}

}  // namespace rtp
