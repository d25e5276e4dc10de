// camera.h — host-side mirror of the reference's Camera / ISaver interface
// (include/camera.cuh:31-84,117-139; src/camera.cu:52-216).  Camera::render() is the drop-in
// point: it calls the MI355X render library through the C ABI (include/rtp_amd.h) where the
// reference launches render_kernel.
#pragma once
#include <cstdint>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rtp_amd.h"
#include "vec_math.h"

namespace rtp {

// ISaver (include/camera.cuh:31-43).  write_color receives the per-pixel SUM of sample
// radiances and divides by the constructor argument — which the reference's drivers set to
// sqrt_rays_per_pixel, not to the sample count (src/camera.cu:300,357): images are sqrt_spp
// times brighter than a mean.  Kept as is for byte parity.
class Saver {
public:
    explicit Saver(int samples_per_pixel) : divisor_(samples_per_pixel) {}
    virtual ~Saver() = default;
    virtual void write_color(Vec3 pixel_sum) = 0;
    virtual void set_format(int width, int height) = 0;
    static float linear_to_gamma(float linear) { return std::sqrt(linear); }  // src/camera.cu:54
    // ÷n → sqrt → clamp[0,0.999] → ×256 → u8 (src/camera.cu:138-147)
    static void quantize(Vec3 pixel_sum, int divisor, uint8_t rgb[3]);

protected:
    int divisor_;
    int width_ = 0, height_ = 0;
};

// FileSaver: ASCII PPM "P3" (src/camera.cu:56-73).
class PpmFileSaver : public Saver {
public:
    PpmFileSaver(int samples_per_pixel, const std::string &filename);
    void write_color(Vec3 pixel_sum) override;
    void set_format(int width, int height) override;
private:
    std::ofstream out_;
};

// OutStreamSaver: the same P3 text on stdout (src/camera.cu:75-92).
class StdoutSaver : public Saver {
public:
    explicit StdoutSaver(int samples_per_pixel) : Saver(samples_per_pixel) {}
    void write_color(Vec3 pixel_sum) override;
    void set_format(int width, int height) override;
};

// PNGSaver (src/camera.cu:94-126): collects RGB8 and writes a PNG when destroyed.  The reference
// compiles it but never instantiates it; its encoder is the third-party stb_image_write, which is
// not part of this repository — png_writer.cpp is a small encoder of its own (same pixels,
// different compressed bytes).
class PngSaver : public Saver {
public:
    PngSaver(int samples_per_pixel, const std::string &filepath);
    ~PngSaver() override;
    void write_color(Vec3 pixel_sum) override;
    void set_format(int width, int height) override;
private:
    std::vector<uint8_t> pixels_;
    std::string path_;
    size_t count_ = 0;
};

// BinarySaver (src/camera.cu:128-153): int32 width, int32 height, then RGB8 rows, top row first.
// This is the saver both reference drivers use (into files NAMED *.png).
class BinarySaver : public Saver {
public:
    BinarySaver(int samples_per_pixel, const std::string &filepath);
    void write_color(Vec3 pixel_sum) override;
    void set_format(int width, int height) override;
private:
    std::ofstream out_;
};

// cudaMemcpyToSymbol(d_scene_data_const, ...) of gpu_render (src/camera.cu:291): the scene every
// later Camera::render() of this thread traces.
void bind_scene(rt_scene *scene);
rt_scene *bound_scene();

// checkCudaErrors (include/camera.cuh:20-29): message on stderr, then exit(99).
void check_rt(rt_status st, const char *expr, const char *file, int line);
#define RTP_CHECK(expr) ::rtp::check_rt((expr), #expr, __FILE__, __LINE__)

class Camera {
public:
    // Argument order (height, width, ...) as in the reference (include/camera.cuh:119-120).
    Camera(int height, int width, std::unique_ptr<Saver> image_saver, Vec3 camera_pos, Vec3 look_at_point = Vec3(0, 0, 0));

    // src/camera.cu:198-216: render the frame into the DEVICE buffer d_fb (width*height*3 floats,
    // per-pixel sums), copy it back and stream every pixel through the saver, row-major.
    void render(float *d_fb) const;
    // src/camera.cu:171-196
    rt_camera_data build_camera_data() const;

    int image_width, image_height;
    float aspect_ratio;
    int samples_per_pixel = 300;
    int max_depth = 50;
    Vec3 background_color{0, 0, 0};
    float vfov = 60.0f;
    std::unique_ptr<Saver> saver;
    Vec3 origin, look_at;
    mutable rt_timing last_timing{};  // kernel time of the last render() (not in the reference)

private:
    Vec3 vup_{0, 0, 1};  // z-up, fixed (src/camera.cu:164)
};

struct SceneParams;
// Eye / look-at for frame n of num_frames (src/camera.cu:301-315).
void orbit_pose(const SceneParams &p, int frame, Vec3 &eye, Vec3 &target);
// … the same orbit at a fractional frame (the shutter of rtp_main --motion-blur); orbit_pose(n) is orbit_pose_at((float)n)
void orbit_pose_at(const SceneParams &p, float frame_time, Vec3 &eye, Vec3 &target);

// gpu_render (src/camera.cu:290-349): per frame BinarySaver + orbit camera + render, printing
// "n \t ms \t W*H*sqrt_spp^2".  The scene must already be bound.  aov (rtp_main --gpu --aov): each frame's first-hit AOVs
// (rt_render_aov) go to "<frame file>.aov" as well (write_aov_file).  denoise (rtp_main --gpu --denoise): each frame is also
// filtered by rt_denoise, guided by its AOVs, and written through a BinarySaver with the frame's own divisor to
// "<frame file>.denoised".  temporal (rtp_main --gpu --denoise-temporal): that file comes from rt_denoise_temporal instead, with the
// history carried from frame to frame (frame 0 starts without one).  The extras run outside the frame's timed span.
void gpu_render(const SceneParams &params, bool aov = false, bool denoise = false, bool temporal = false);

// The .aov file of a frame: int32 width, height, spp, then per pixel in row order 8 float32 — albedo_sum / spp (3),
// normal_sum / spp (3), depth_sum / hit_count (0 where no sample hit) and hit_count / spp, each one float32 division.
// Inputs as rt_aov_buffers holds them (width * height pixels).  Returns false when the file cannot be written.
bool write_aov_file(const std::string &path, int32_t width, int32_t height, int32_t spp, const float *albedo_sum, const float *normal_sum,
                    const float *depth_sum, const uint32_t *hit_count);

// Animation driver beyond the reference: frames dealt round-robin to num_devices GPUs, saver
// arithmetic on the device, file output overlapped with the next frame.  Same files, byte for byte.
void gpu_render_pipelined(const SceneParams &params, const rt_scene_desc &desc, int num_devices);
// What gpu_render_lens and gpu_render_adaptive render, member by member (rtp_main fills one from its command line).  The
// pointers are borrowed for the call; a null pointer or a false flag is that feature off.
struct FrameJob {
    const rt_lens_params *lens = nullptr;          // rtp_main --lens R:F: the thin lens; null: rt_lens_params_init's pinhole
    float shutter = 0.0f;                          // --motion-blur S: open at frame n, closed at n + S; 0: no motion
    bool aov = false;                              // --aov: each frame's first-hit AOVs to "<frame file>.aov" (from rt_render_aov_lens)
    bool denoise = false;                          // --denoise: each frame also filtered by rt_denoise to "<frame file>.denoised"
    const rt_nee_params *nee = nullptr;            // --nee: frames through rt_render_nee (the lens and shutter then unused: a pinhole at frame n)
    const rt_env *env = nullptr;                   // --env: through rt_render_env with env_params, likewise
    const rt_env_params *env_params = nullptr;
    // --lit: through rt_render_lit with lit's emitters and environment, this lens and this shutter (lit->lens and lit->cam_close are set
    // per frame by the driver), aov / denoise from rt_render_aov_lens
    const rt_lit_params *lit = nullptr;
    // with lit, --lit --noise-target: through rt_render_lit_adaptive and rt_tonemap_spp.  gpu_render_adaptive (--adaptive T): its
    // parameters, never null there
    const rt_adaptive_params *noise = nullptr;
    // with noise, --denoise-adaptive: each frame also filtered by rt_denoise_spp with its counts and moments and AOVs at noise->min_spp
    // (rt_render_aov_lens; gpu_render_adaptive: rt_render_aov), written through rt_tonemap_spp to "<frame file>.denoised"
    bool denoise_adaptive = false;
    const rt_stop_params *stop = nullptr;          // --stop-rule: the stopping rule of the adaptive frames; null: the pixel's own error
    // with noise, a pinhole and a closed shutter, --denoise-adaptive-temporal: that file from rt_denoise_temporal_spp instead, the AOVs
    // (first_prim included) from rt_render_aov at noise->min_spp and the two histories swapped per frame
    bool denoise_adaptive_temporal = false;
    const rt_medium_params *medium = nullptr;      // --fog: the lit frames through rt_render_medium
    // with denoise_adaptive_temporal, --stop-history: those AOVs first, rt_adaptive_prior on the previous frame's history, the frame
    // through rt_render_lit_adaptive_prior (gpu_render_adaptive: rt_render_adaptive_prior)
    bool stop_history = false;
    // with medium, --fog-grid: through rt_render_volume, this grid in the medium's box; medium with noise (--fog-noise-target): through
    // rt_render_volume_adaptive (volume may be null) and rt_tonemap_spp
    const rt_volume *volume = nullptr;
    // with medium, --fog-denoise: each frame also filtered under rt_render_aov_volume's AOVs — by rt_denoise, or with noise by
    // rt_denoise_spp with the frame's counts and moments and AOVs at noise->min_spp — to "<frame file>.denoised"
    bool fog_denoise = false;
    // with lit alone (no noise, no medium), --split: through rt_render_lit_split — "<frame file>.direct" and "<frame file>.indirect" in the frame's
    // own format, the frame from their float32 sum, and with denoise "<frame file>.denoised" from rt_denoise_split
    bool split = false;
    const rt_chroma_params *chroma = nullptr;      // with medium, --fog-tint: the lit frames through rt_render_chroma, with or without the volume
    const rt_glow_params *glow = nullptr;          // with medium, without chroma, --fog-glow: through rt_render_glow, with or without the volume
    const rt_volume *heat = nullptr;               // the grid of glow's source 2 (--fog-heat)
    const rt_glow_sample_params *glow_sample = nullptr;          // with glow and volume, --fog-glow-sample: through rt_render_glow_sampled …
    const rt_glow_sampler *sampler = nullptr;                    // … with the sampler of these grids
    // with medium, --fog-adaptive: through rt_render_fog_adaptive with volume, chroma, glow, heat, glow_sample and sampler as they stand
    // here, and rt_tonemap_spp; without a stop rule or a prior
    const rt_adaptive_params *fog_adaptive = nullptr;
};
// rtp_main --gpu --lens R:F / --motion-blur S / --nee / --env / --lit: the orbit frame after frame on one GPU through the render call the
// job's members pick (rt_render_lens when none does), saved with rt_tonemap
void gpu_render_lens(const SceneParams &params, const rt_scene_desc &desc, const FrameJob &job);
// rtp_main --gpu --adaptive: the orbit frame after frame on one GPU, each frame through rt_render_adaptive and rt_tonemap_spp.  Reads
// job.noise, denoise_adaptive, stop, denoise_adaptive_temporal and stop_history
void gpu_render_adaptive(const SceneParams &params, const rt_scene_desc &desc, const FrameJob &job);

// … and the other split: every frame sharded in row bands over num_devices GPUs (<= 0: all) with one RCCL gather per
// frame (rt_context, rt_render_sharded).  Same files, byte for byte.
void gpu_render_sharded(const SceneParams &params, const rt_scene_desc &desc, int num_devices);

}  // namespace rtp
