// cli.h — rtp_main's command line, read once.  parse_cli walks argv one time, then runs one ordered list of refusals
// and names the driver an accepted command line goes to.  Plain values only: nothing here (or in cli.cpp) calls the render library or
// needs a device, so a command line is judged before any device object is made.
//
// The flags behind `rtp_main --gpu` (extensions beyond the reference; which flag needs and excludes which is the list in cli.cpp):
//   --aov | --denoise | --denoise-temporal      "<frame file>.aov"; "<frame file>.denoised" from rt_denoise / rt_denoise_temporal
//   --devices N (or RTP_DEVICES=N) | --shard N  the pipelined multi-GPU driver | every frame split over N GPUs (0: all of the node)
//   --adaptive T [--adaptive-spp min:batch:max] rt_render_adaptive and rt_tonemap_spp (default 16:16:256)
//   --lens R:F, --motion-blur S                 rt_render_lens: thin lens of radius R focused at F; shutter open from frame n to n + S
//   --nee [mis|light] [--light-tree]            rt_render_nee: light samples of the emitters; the emitter picked by the light tree
//   --env FILE[:N] [--env-mode path|mis|light] [--env-scale S] [--env-up y|z]   rt_render_env: a PFM / .hdr lat-long image as an N x N map
//   --glossy                                    with --nee, --env (mis, light) or --lit: METAL's reflect branch takes light samples too
//   --lit                                       rt_render_lit: --nee, --env, --lens and --motion-blur in any combination, and with it only
//   --lit --noise-target T [--noise-spp min:batch:max]                          rt_render_lit_adaptive
//   --lit --split                               rt_render_lit_split: "<frame file>.direct" and "<frame file>.indirect" beside the frame, which is
//                                               saved from their sum; with --denoise, "<frame file>.denoised" from rt_denoise_split
//   --denoise-adaptive | --denoise-adaptive-temporal [--stop-history], --stop-rule own|near    with --adaptive or --lit --noise-target:
//                                               rt_denoise_spp | rt_denoise_temporal_spp [its history as the prior]; the stopping rule
//   --lit --fog SIGMA[:ALBEDO[:G]] [--fog-ball cx,cy,cz,r | --fog-box x0,y0,z0,x1,y1,z1]       rt_render_medium
//     --fog-grid FILE                           (with --fog-box) rt_render_volume: "VOL1\nnx ny nz\n", then nx*ny*nz float32, x fastest
//     --fog-tint R,G,B                          rt_render_chroma
//     --fog-glow R,G,B[:density] [--fog-heat FILE] [--fog-glow-sample mis|light]               rt_render_glow / rt_render_glow_sampled
//     --fog-noise-target T[:min:batch:max]      rt_render_volume_adaptive
//     --fog-adaptive T[:min:batch:max]          rt_render_fog_adaptive: a noise target with --fog-tint, --fog-glow, --fog-glow-sample too
//     --fog-denoise                             the fogged frame filtered under rt_render_aov_volume's AOVs
#pragma once
#include <string>
#include <vector>

#include "texture_io.h"

namespace rtp {

// min:batch:max of --adaptive-spp, --noise-spp and --fog-noise-target / --fog-adaptive T:min:batch:max; not given: rt_adaptive_params_init's triple stands
struct CliSpp {
    bool given = false;
    int min_spp = 0, batch_spp = 0, max_spp = 0;
};

// A --fog-grid / --fog-heat file: n[0] * n[1] * n[2] cells, x fastest; empty: no such file was asked for
struct CliGrid {
    std::vector<float> cells;
    int n[3] = {0, 0, 0};
};

struct Cli {
    // which frame driver of camera.h renders: gpu_render, gpu_render_lens, gpu_render_adaptive, gpu_render_sharded, gpu_render_pipelined
    enum class Driver { frames, lens, adaptive, sharded, pipelined };
    Driver driver = Driver::frames;

    // the flags that are on (each: the element is somewhere in argv)
    bool aov = false, denoise = false, denoise_temporal = false, denoise_adaptive = false, denoise_adaptive_temporal = false;
    bool stop_history = false, lit = false, glossy = false, light_tree = false, nee = false, env = false;
    bool fog = false, fog_denoise = false, fog_tint = false, fog_glow = false, fog_glow_sample = false, fog_noise = false, fog_adaptive = false, noise = false;
    bool lens = false, motion_blur = false;
    bool split = false;                                     // --split (with --lit only)

    int stop_rule = 0;                                      // --stop-rule: 0 own (default), 1 near
    // --fog SIGMA[:ALBEDO[:G]], --fog-ball / --fog-box (read when fog)
    float fog_sigma = 0.0f, fog_albedo = 1.0f, fog_g = 0.0f;
    int fog_region = 0;                                     // 0 all space, 1 ball (a, b[0]), 2 box (a, b)
    float fog_a[3] = {0, 0, 0}, fog_b[3] = {0, 0, 0};
    CliGrid fog_grid, fog_heat;                             // --fog-grid FILE, --fog-heat FILE
    float fog_tint_rgb[3] = {1, 1, 1};                      // --fog-tint R,G,B (read when fog_tint)
    float fog_glow_radiance[3] = {0, 0, 0};                 // --fog-glow R,G,B[:density] (read when fog_glow)
    int fog_glow_source = 0;                                // 0 uniform, 1 :density, 2 --fog-heat
    int fog_glow_sample_mis = 1;                            // --fog-glow-sample mis (1) | light (0)
    float fog_noise_threshold = 0.0f, noise_threshold = 0.0f, adaptive_threshold = 0.0f;          // (read when fog_noise / noise / driver adaptive)
    CliSpp fog_noise_spp, noise_spp, adaptive_spp;
    float fog_adaptive_threshold = 0.0f;                    // --fog-adaptive T[:min:batch:max] (read when fog_adaptive)
    CliSpp fog_adaptive_spp;
    // --env FILE[:N] --env-mode --env-scale --env-up (read when env)
    std::string env_file;
    int env_n = 1024;
    int env_mode = -1;                                      // 0 path, 1 mis, 2 light; -1: not given, rt_env_params_init's stands
    bool env_scale_given = false;
    float env_scale = 0.0f;
    bool env_up_z = false;
    HdrImage env_image;                                     // FILE, loaded
    int nee_mis = -1;                                       // --nee mis (1) | light (0); -1: no word, rt_nee_params_init's stands
    float lens_radius = 0.0f, lens_focus = 0.0f, shutter = 0.0f;          // --lens R:F (read when lens), --motion-blur S (0: closed)
    int devices = 0, shards = 0;                            // driver pipelined: GPUs; driver sharded: GPUs (<= 0: all)
};

struct CliRefusal {
    int code = 0;           // rtp_main's exit code: 2 or 99
    std::string text;       // the line after "rtp_main: "
};

// argv as main() got it (argv[1] is the mode word, the flags start at argv[2]); rtp_devices: the value of RTP_DEVICES, null when unset.
// false: refused, and `refusal` says how.  Reads the files the command line names (grid, heat, environment image), writes none.
bool parse_cli(int argc, const char *const *argv, const char *rtp_devices, Cli &cli, CliRefusal &refusal);

}  // namespace rtp
