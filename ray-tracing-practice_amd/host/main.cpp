// main.cpp — CLI with the reference's modes (src/main.cu:572-606): no argument or --gpu reads a
// scene description from stdin and renders every frame on the GPU; --default prints the default
// description.  --cpu is the reference's single-threaded CPU loop: this build ships no CPU
// render path (its CPU restatement lives under oracle/ as a test checker only), so --cpu fails
// loudly instead of silently rendering on the host.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "camera.h"
#include "scene_builder.h"
#include "scene_params.h"
#include "texture_io.h"

// A grid file of --fog-grid and --fog-heat: the ASCII header "VOL1\nnx ny nz\n" and then exactly nx * ny * nz little-endian float32 (this
// build's hosts are little-endian, like the file), finite and not negative, x fastest
static bool read_grid_file(const std::string &file, int n[3], std::vector<float> &grid) {
    FILE *f = file.empty() ? nullptr : fopen(file.c_str(), "rb");
    char magic[8] = {0}, eol = 0;
    size_t count = 0;
    bool ok = f && fgets(magic, sizeof(magic), f) && std::strcmp(magic, "VOL1\n") == 0 && fscanf(f, "%d %d %d%c", &n[0], &n[1], &n[2], &eol) == 4 && eol == '\n';
    for (int k = 0; ok && k < 3; ++k) ok = n[k] >= 1 && n[k] <= RT_VOLUME_MAX_N;
    if (ok) {
        count = static_cast<size_t>(n[0]) * n[1] * n[2];
        grid.resize(count);
        ok = fread(grid.data(), sizeof(float), count, f) == count && fgetc(f) == EOF;
    }
    for (size_t k = 0; ok && k < count; ++k) ok = std::isfinite(grid[k]) && grid[k] >= 0.0f;
    if (f) fclose(f);
    return ok;
}

int main(int argc, char *argv[]) {
    const std::string mode = argc < 2 ? "--gpu" : argv[1];
    if (mode == "--default") {
        std::cout << rtp::default_config_text();
        return 0;
    }
    if (mode == "--cpu") {
        std::cerr << "rtp_main: --cpu is not available: this build renders on an MI355X only\n";
        return 2;
    }
    if (mode != "--gpu") return 0;  // unknown arguments are ignored by the reference too

    rtp::SceneParams params = rtp::read_scene_params(std::cin);
    rtp::HostScene host;
    rtp::build_config_scene(params, "", host);

    const rt_scene_desc desc = host.desc();
    // extension: `--gpu --aov` also writes each frame's first-hit AOVs to "<frame file>.aov", and `--gpu --denoise` the frame filtered
    // by rt_denoise to "<frame file>.denoised"; `--gpu --denoise-temporal` writes that file through rt_denoise_temporal instead, the
    // history carried from frame to frame (frame-after-frame driver only)
    bool aov = false, denoise = false, temporal = false;
    for (int a = 2; a < argc; ++a) {
        if (std::string(argv[a]) == "--aov") aov = true;
        if (std::string(argv[a]) == "--denoise") denoise = true;
        if (std::string(argv[a]) == "--denoise-temporal") temporal = true;
    }
    // extension: `--lit … --fog SIGMA … --fog-denoise`, with or without --fog-ball, --fog-box, --fog-grid and --fog-noise-target:
    // each fogged frame is also filtered under the fog-aware AOVs of rt_render_aov_volume — by rt_denoise, or with --fog-noise-target by
    // rt_denoise_spp with the frame's counts and moments and AOVs at min_spp — and written through the frame's own saver to
    // "<frame file>.denoised".  The flag needs --fog and is not for --denoise*, --aov, --adaptive, --devices or --shard.  This block comes
    // before those flags' own, so that whatever else is given the refusal names this flag.
    bool fog_denoise = false;
    {
        bool fog_flag = false;
        std::string other;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--fog-denoise") fog_denoise = true;
            if (arg == "--fog") fog_flag = true;
            if (arg.compare(0, 9, "--denoise") == 0 || arg == "--aov" || arg == "--adaptive" || arg == "--devices" || arg == "--shard") other = arg;
        }
        std::string bad;
        if (fog_denoise && !fog_flag) bad = "--fog-denoise filters fogged frames: it needs --lit --fog SIGMA";
        else if (fog_denoise && !other.empty())
            bad = "--fog-denoise cannot be combined with " + other + " (not with --denoise*, --aov, --adaptive, --devices or --shard)";
        if (!bad.empty()) {
            std::cerr << "rtp_main: " << bad << "\n";
            return 99;
        }
    }
    // extension: `--lit … --fog SIGMA … [--fog-ball | --fog-box …] [--fog-grid FILE] --fog-glow R,G,B[:density] [--fog-heat FILE]`:
    // the fogged frames through rt_render_glow — the medium emits R,G,B per unit length, uniformly over its region, scaled cell by cell by
    // the density grid (`:density`) or by a second grid (--fog-heat FILE, --fog-grid's format and dimensions).  The flag needs --fog and is
    // not for --fog-tint, --fog-noise-target or --fog-denoise: no chroma, adaptive, AOV or denoise call takes a glow.  This block comes
    // before those flags' own, so that the refusal names this flag.  (The heat file is read below, after the grid's.)
    // `--fog-glow … --fog-grid FILE --fog-glow-sample mis|light`: through rt_render_glow_sampled — the glow is light-sampled,
    // with the power heuristic (mis) or alone (light).  The flag needs --fog-glow and --fog-grid: the sample picks a cell of the grid.
    bool fog_glow_on = false, fog_glow_sample_on = false;
    rt_glow_params fog_glow;
    rt_glow_params_init(&fog_glow);
    rt_glow_sample_params fog_glow_sample;
    rt_glow_sample_params_init(&fog_glow_sample);
    std::string fog_heat_file;
    {
        bool fog_flag = false, grid_flag = false, heat_flag = false, by_density = false;
        std::string bad, other;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--fog") fog_flag = true;
            if (arg == "--fog-grid") grid_flag = true;
            if (arg == "--fog-tint" || arg == "--fog-noise-target" || arg == "--fog-denoise") other = arg;
            if (arg == "--fog-heat") {
                heat_flag = true;
                fog_heat_file = a + 1 < argc ? argv[a + 1] : "";
            }
            if (arg == "--fog-glow-sample") {
                fog_glow_sample_on = true;
                const std::string value = a + 1 < argc ? argv[a + 1] : "";
                if (value != "mis" && value != "light") bad = "--fog-glow-sample takes mis or light";
                fog_glow_sample.sample = 1;
                fog_glow_sample.mis = value == "light" ? 0 : 1;
            }
            if (arg == "--fog-glow") {
                fog_glow_on = true;
                std::string value = a + 1 < argc ? argv[a + 1] : "";
                const std::string suffix = ":density";
                by_density = value.size() > suffix.size() && value.compare(value.size() - suffix.size(), suffix.size(), suffix) == 0;
                if (by_density) value.resize(value.size() - suffix.size());
                char tail = 0;
                bool ok = sscanf(value.c_str(), "%f,%f,%f%c", &fog_glow.radiance[0], &fog_glow.radiance[1], &fog_glow.radiance[2], &tail) == 3;
                for (int k = 0; ok && k < 3; ++k) ok = std::isfinite(fog_glow.radiance[k]) && fog_glow.radiance[k] >= 0.0f;
                if (!ok) bad = "--fog-glow takes R,G,B[:density]: three finite numbers, none negative";
            }
        }
        if (heat_flag && !fog_glow_on && bad.empty()) bad = "--fog-heat shapes the emission of --fog-glow: it needs --fog-glow R,G,B";
        if (fog_glow_on && bad.empty() && !fog_flag) bad = "--fog-glow makes the medium of --fog emit: it needs --lit --fog SIGMA with SIGMA > 0";
        if (fog_glow_on && bad.empty() && !other.empty())
            bad = "--fog-glow cannot be combined with " + other + ": the chroma, adaptive, AOV and denoise calls take no glow";
        if (fog_glow_on && bad.empty() && heat_flag && by_density) bad = "--fog-glow R,G,B:density and --fog-heat exclude each other: the emission follows one grid";
        if (fog_glow_on && bad.empty() && by_density && !grid_flag) bad = "--fog-glow R,G,B:density follows the density grid: it needs --fog-grid FILE";
        if (fog_glow_on && bad.empty() && heat_flag && !grid_flag) bad = "--fog-heat has the dimensions of the density grid: it needs --fog-grid FILE";
        if (fog_glow_sample_on && bad.empty() && !fog_glow_on) bad = "--fog-glow-sample aims at the glow: it needs --fog-glow R,G,B";
        if (fog_glow_sample_on && bad.empty() && !grid_flag)
            bad = "--fog-glow-sample picks a cell of the density grid: it needs --fog-grid FILE (a homogeneous box can pass a 1 x 1 x 1 grid)";
        if (!bad.empty()) {
            std::cerr << "rtp_main: " << bad << "\n";
            return 99;
        }
        fog_glow.source = heat_flag ? 2 : (by_density ? 1 : 0);
    }
    // extension: `--lit … --fog SIGMA … [--fog-ball | --fog-box …] [--fog-grid FILE] --fog-tint R,G,B`: the fogged frames through
    // rt_render_chroma — the extinction of colour channel k is SIGMA times its tint.  The flag needs --fog and is not for --fog-noise-target or
    // --fog-denoise: no adaptive, AOV or denoise call takes a tint.  This block comes before those flags' own, so that the refusal names this flag.
    bool fog_tint_on = false;
    rt_chroma_params fog_tint;
    rt_chroma_params_init(&fog_tint);
    {
        bool fog_flag = false;
        std::string bad, other;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--fog") fog_flag = true;
            if (arg == "--fog-noise-target" || arg == "--fog-denoise") other = arg;
            if (arg == "--fog-tint") {
                fog_tint_on = true;
                char tail = 0;
                bool ok = sscanf(a + 1 < argc ? argv[a + 1] : "", "%f,%f,%f%c", &fog_tint.tint[0], &fog_tint.tint[1], &fog_tint.tint[2], &tail) == 3;
                for (int k = 0; ok && k < 3; ++k) ok = std::isfinite(fog_tint.tint[k]) && fog_tint.tint[k] >= 0.0f;
                if (!ok) bad = "--fog-tint takes R,G,B: three finite numbers, none negative";
            }
        }
        if (fog_tint_on && bad.empty() && !fog_flag) bad = "--fog-tint colours the extinction of --fog: it needs --lit --fog SIGMA";
        if (fog_tint_on && bad.empty() && !other.empty())
            bad = "--fog-tint cannot be combined with " + other + ": the adaptive, AOV and denoise calls take no tint (grey fog only)";
        if (!bad.empty()) {
            std::cerr << "rtp_main: " << bad << "\n";
            return 99;
        }
    }
    // extension: `--lit … --fog SIGMA … [--fog-grid FILE] --fog-noise-target T[:min:batch:max]`: the fogged frames through
    // rt_render_volume_adaptive (adaptive sampling under the medium or the grid, default 16:16:256) and rt_tonemap_spp.  The flag needs --fog
    // and is not for --adaptive, --denoise*, --aov, --stop-rule, --stop-history or --noise-target.  This block comes before those flags' own,
    // so that whatever else is given the refusal names this flag.
    bool fog_noise_on = false;
    rt_adaptive_params fog_noise;
    rt_adaptive_params_init(&fog_noise);
    {
        bool fog_flag = false;
        std::string bad, other;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--fog") fog_flag = true;
            if (arg == "--adaptive" || arg.compare(0, 9, "--denoise") == 0 || arg == "--aov" || arg == "--stop-rule" || arg == "--stop-history" ||
                arg == "--noise-target")
                other = arg;
            if (arg == "--fog-noise-target") {
                fog_noise_on = true;
                const char *value = a + 1 < argc ? argv[a + 1] : "";
                char *end = nullptr;
                fog_noise.threshold = strtof(value, &end);
                bool ok = end != value && std::isfinite(fog_noise.threshold) && fog_noise.threshold >= 0.0f;
                if (ok && *end == ':') {
                    char tail = 0;
                    ok = sscanf(end + 1, "%d:%d:%d%c", &fog_noise.min_spp, &fog_noise.batch_spp, &fog_noise.max_spp, &tail) == 3 && fog_noise.min_spp >= 2 &&
                         fog_noise.batch_spp >= 1 && fog_noise.max_spp >= fog_noise.min_spp && fog_noise.max_spp <= 65536;
                } else if (ok) {
                    ok = *end == 0;
                }
                if (!ok)
                    bad = "--fog-noise-target takes T[:min:batch:max] with T finite and not negative, min >= 2, batch >= 1 and min <= max <= 65536";
            }
        }
        if (fog_noise_on && bad.empty() && !fog_flag) bad = "--fog-noise-target sets the noise target of fogged frames: it needs --lit --fog SIGMA";
        if (fog_noise_on && bad.empty() && !other.empty())
            bad = "--fog-noise-target cannot be combined with " + other + " (not with --adaptive, --denoise*, --aov, --stop-rule, --stop-history or --noise-target)";
        if (!bad.empty()) {
            std::cerr << "rtp_main: " << bad << "\n";
            return 99;
        }
    }
    // extension: `--denoise-adaptive-temporal`, with `--adaptive T` or with `--lit … --noise-target T` (pinhole frames only: the
    // reprojection assumes one): --denoise-adaptive with the history carried from frame to frame — rt_denoise_temporal_spp with each
    // frame's counts and moments and AOVs (first_prim included) at min_spp, through rt_tonemap_spp to "<frame file>.denoised".  Not
    // with --denoise, --denoise-temporal, --denoise-adaptive, --aov, --lens, --motion-blur, --devices, --shard or RTP_DEVICES: this
    // block comes before those flags' own, so that whatever else is given the refusal names this flag.
    bool denoise_adaptive_temporal = false;
    {
        bool adaptive_on = false, lit_flag = false, target_flag = false, others = getenv("RTP_DEVICES") != nullptr;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--denoise-adaptive-temporal") denoise_adaptive_temporal = true;
            if (arg == "--adaptive") adaptive_on = true;
            if (arg == "--lit") lit_flag = true;
            if (arg == "--noise-target") target_flag = true;
            if (arg == "--denoise-adaptive" || arg == "--lens" || arg == "--motion-blur" || arg == "--devices" || arg == "--shard") others = true;
        }
        if (denoise_adaptive_temporal && (denoise || temporal || aov || others)) {
            std::cerr << "rtp_main: --denoise-adaptive-temporal writes <frame>.denoised from pinhole frames and AOVs of its own on one GPU: it cannot "
                         "be combined with --denoise, --denoise-temporal, --denoise-adaptive, --aov, --lens, --motion-blur, --devices, --shard or "
                         "RTP_DEVICES\n";
            return 2;
        }
        if (denoise_adaptive_temporal && !adaptive_on && !(lit_flag && target_flag)) {
            std::cerr << "rtp_main: --denoise-adaptive-temporal filters adaptively sampled frames: it needs --adaptive T or --lit --noise-target T\n";
            return 2;
        }
    }
    // extension: `--stop-history`, only with `--denoise-adaptive-temporal`: each frame's AOVs at min_spp are rendered
    // first, rt_adaptive_prior makes the prior from the previous frame's history (none on frame 0) and the frame goes through
    // rt_render_adaptive_prior / rt_render_lit_adaptive_prior; the denoiser runs as without the flag.
    bool stop_history = false;
    for (int a = 2; a < argc; ++a)
        if (std::string(argv[a]) == "--stop-history") stop_history = true;
    if (stop_history && !denoise_adaptive_temporal) {
        std::cerr << "rtp_main: --stop-history feeds the history of --denoise-adaptive-temporal back into the stopping rule: it needs that flag\n";
        return 2;
    }
    // extension: `--denoise-adaptive`, with `--adaptive T` or with `--lit … --noise-target T` and only with them: each adaptively sampled
    // frame is also filtered by rt_denoise_spp — its own counts and moments, AOVs rendered at min_spp (rt_render_aov; on the lit path
    // rt_render_aov_lens with the frame's lens and shutter) — and written through rt_tonemap_spp to "<frame file>.denoised".  Not with
    // --denoise, --denoise-temporal or --aov.
    bool denoise_adaptive = false;
    {
        bool adaptive_on = false, lit_flag = false, target_flag = false;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--denoise-adaptive") denoise_adaptive = true;
            if (arg == "--adaptive") adaptive_on = true;
            if (arg == "--lit") lit_flag = true;
            if (arg == "--noise-target") target_flag = true;
        }
        if (denoise_adaptive && (denoise || temporal || aov)) {
            std::cerr << "rtp_main: --denoise-adaptive writes <frame>.denoised from AOVs of its own: it cannot be combined with --denoise, "
                         "--denoise-temporal or --aov\n";
            return 2;
        }
        if (denoise_adaptive && !adaptive_on && !(lit_flag && target_flag)) {
            std::cerr << "rtp_main: --denoise-adaptive filters adaptively sampled frames: it needs --adaptive T or --lit --noise-target T\n";
            return 2;
        }
    }
    // extension: `--stop-rule own|near`, with `--adaptive T` or with `--lit … --noise-target T` and only with them: the stopping rule of
    // the adaptive frames (rt_render_adaptive_rule / rt_render_lit_adaptive_rule).  own, the default: the pixel's own
    // relative error — the frames without the flag; near: the neighbourhood rule.
    rt_stop_params stop_rule;
    rt_stop_params_init(&stop_rule);
    {
        bool adaptive_on = false, lit_flag = false, target_flag = false, given = false;
        std::string word;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--adaptive") adaptive_on = true;
            if (arg == "--lit") lit_flag = true;
            if (arg == "--noise-target") target_flag = true;
            if (arg == "--stop-rule") {
                given = true;
                word = a + 1 < argc ? argv[a + 1] : "";
            }
        }
        if (given && word != "own" && word != "near") {
            std::cerr << "rtp_main: --stop-rule takes own or near\n";
            return 2;
        }
        if (given && !adaptive_on && !(lit_flag && target_flag)) {
            std::cerr << "rtp_main: --stop-rule picks the stopping rule of adaptively sampled frames: it needs --adaptive T or --lit --noise-target T\n";
            return 2;
        }
        stop_rule.rule = word == "near" ? 1 : 0;
    }
    // extension: `--gpu --lit`: every frame through rt_render_lit on one GPU — light samples of the emissive spheres (`--nee [mis|light]`
    // picks their weighting), and with it, and only with it, `--env FILE[:N]` (with --env-mode, --env-scale, --env-up), `--lens R:F` and
    // `--motion-blur S` in any combination; --aov / --denoise as with --lens (first hits do not depend on the estimator).  Each of those
    // flags is parsed by its own block below, which hands its value on instead of rendering.  Not with --adaptive, --denoise-temporal,
    // --devices, --shard or RTP_DEVICES.
    // `--lit --noise-target T [--noise-spp min:batch:max]`: those frames through rt_render_lit_adaptive (adaptive sampling on the lit path,
    // default 16:16:256) and rt_tonemap_spp.  --noise-target needs --lit and is not for --adaptive, --denoise or --aov; --noise-spp needs
    // --noise-target.
    bool lit_on = false, noise_on = false;
    rt_adaptive_params noise;
    rt_adaptive_params_init(&noise);
    rt_env *lit_env = nullptr;
    rt_env_params lit_ep;
    rt_env_params_init(&lit_ep);
    rt_nee_params lit_nee;
    rt_nee_params_init(&lit_nee);
    {
        bool lit_others = getenv("RTP_DEVICES") != nullptr;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--lit") lit_on = true;
            if (arg == "--adaptive" || arg == "--denoise-temporal" || arg == "--devices" || arg == "--shard") lit_others = true;
        }
        bool noise_spp = false, noise_adaptive = false;
        std::string noise_bad;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            const std::string value = a + 1 < argc ? argv[a + 1] : "";
            if (arg == "--adaptive") noise_adaptive = true;
            if (arg == "--noise-target") {
                noise_on = true;
                char *end = nullptr;
                noise.threshold = strtof(value.c_str(), &end);
                if (value.empty() || *end != 0 || !(std::isfinite(noise.threshold) && noise.threshold >= 0.0f))
                    noise_bad = "--noise-target takes a finite threshold that is not negative";
            }
            if (arg == "--noise-spp") {
                noise_spp = true;
                char tail = 0;
                if (sscanf(value.c_str(), "%d:%d:%d%c", &noise.min_spp, &noise.batch_spp, &noise.max_spp, &tail) != 3 || noise.min_spp < 2 ||
                    noise.batch_spp < 1 || noise.max_spp < noise.min_spp || noise.max_spp > 65536)
                    noise_bad = "--noise-spp takes min:batch:max with min >= 2, batch >= 1 and min <= max <= 65536";
            }
        }
        if (noise_spp && !noise_on) noise_bad = "--noise-spp needs --noise-target T";
        else if (noise_on && !lit_on) noise_bad = "--noise-target sets the noise target of --lit frames: it needs --lit";
        else if (noise_on && noise_bad.empty() && (noise_adaptive || aov || denoise))
            noise_bad = "--noise-target cannot be combined with --adaptive, --denoise or --aov";
        if (!noise_bad.empty()) {
            std::cerr << "rtp_main: " << noise_bad << "\n";
            return 99;
        }
        if (lit_on && lit_others) {
            std::cerr << "rtp_main: --lit renders frame after frame on one GPU: it cannot be combined with --adaptive, --denoise-temporal, "
                         "--devices, --shard or RTP_DEVICES\n";
            return 99;
        }
    }
    // extension: `--lit … --fog SIGMA[:ALBEDO[:G]] [--fog-ball cx,cy,cz,r | --fog-box x0,y0,z0,x1,y1,z1]`: the --lit frames through
    // rt_render_medium — a homogeneous grey medium of extinction SIGMA, single-scattering albedo ALBEDO (default 1) and Henyey-Greenstein g
    // G (default 0) in all space, a ball or a box.  --fog needs --lit and is not for --noise-target (adaptive sampling under
    // a medium is --fog-noise-target, above); --fog-ball / --fog-box need --fog and exclude each other.
    // `--fog-grid FILE` (with --fog-box): the frames through rt_render_volume — the density grid of FILE fills the box and scales SIGMA cell
    // by cell.  FILE is the ASCII header "VOL1\nnx ny nz\n" and then nx * ny * nz little-endian float32, x fastest.
    bool fog_on = false;
    rt_medium_params fog;
    rt_medium_params_init(&fog);
    std::vector<float> fog_grid, fog_heat;
    int fog_n[3] = {0, 0, 0}, fog_heat_n[3] = {0, 0, 0};
    {
        bool ball = false, box = false, grid = false;
        std::string grid_file;
        std::string fog_bad;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            const char *value = a + 1 < argc ? argv[a + 1] : "";
            char tail = 0;
            if (arg == "--fog") {
                fog_on = true;
                float alb = 1.0f, g = 0.0f;
                // one to three numbers between colons, each read to its end
                float *into[3] = {&fog.sigma_t, &alb, &g};
                int got = 0;
                bool ok = *value != 0;
                for (const char *at = value; ok; ++got) {
                    char *end = nullptr;
                    if (got == 3) { ok = false; break; }
                    *into[got] = strtof(at, &end);
                    ok = end != at && (*end == 0 || *end == ':');
                    if (!ok || *end == 0) { ++got; break; }
                    at = end + 1;
                }
                if (!ok || !(std::isfinite(fog.sigma_t) && fog.sigma_t >= 0.0f) || !(alb >= 0.0f && alb <= 1.0f) || !(std::fabs(g) <= 0.95f))
                    fog_bad = "--fog takes SIGMA[:ALBEDO[:G]] with SIGMA >= 0 and finite, 0 <= ALBEDO <= 1 and |G| <= 0.95";
                fog.albedo[0] = fog.albedo[1] = fog.albedo[2] = alb;
                fog.g = g;
            }
            if (arg == "--fog-ball") {
                ball = true;
                fog.region = 1;
                if (sscanf(value, "%f,%f,%f,%f%c", &fog.a[0], &fog.a[1], &fog.a[2], &fog.b[0], &tail) != 4 || !(fog.b[0] > 0.0f) || !std::isfinite(fog.b[0]) ||
                    !std::isfinite(fog.a[0]) || !std::isfinite(fog.a[1]) || !std::isfinite(fog.a[2]))
                    fog_bad = "--fog-ball takes cx,cy,cz,r with finite numbers and r > 0";
            }
            if (arg == "--fog-box") {
                box = true;
                fog.region = 2;
                bool ok = sscanf(value, "%f,%f,%f,%f,%f,%f%c", &fog.a[0], &fog.a[1], &fog.a[2], &fog.b[0], &fog.b[1], &fog.b[2], &tail) == 6;
                for (int k = 0; ok && k < 3; ++k) ok = std::isfinite(fog.a[k]) && std::isfinite(fog.b[k]) && fog.a[k] < fog.b[k];
                if (!ok) fog_bad = "--fog-box takes x0,y0,z0,x1,y1,z1 with finite numbers and x0 < x1, y0 < y1, z0 < z1";
            }
            if (arg == "--fog-grid") {
                grid = true;
                grid_file = value;
            }
        }
        if ((ball || box) && !fog_on) fog_bad = "--fog-ball and --fog-box bound the medium of --fog: they need --fog SIGMA";
        else if (ball && box) fog_bad = "--fog-ball and --fog-box exclude each other: the medium has one region";
        else if (fog_on && !lit_on) fog_bad = "--fog puts a medium into --lit frames: it needs --lit";
        else if (fog_on && noise_on) fog_bad = "--fog cannot be combined with --noise-target: adaptive sampling under a medium is --fog-noise-target T";
        else if (grid && ball) fog_bad = "--fog-grid fills a box: it cannot be combined with --fog-ball";
        else if (grid && !box) fog_bad = "--fog-grid fills the box of --fog-box: it needs --fog SIGMA and --fog-box";
        if (fog_bad.empty() && grid) {
            if (!read_grid_file(grid_file, fog_n, fog_grid))
                fog_bad = "--fog-grid takes a FILE of the header \"VOL1\\nnx ny nz\\n\" (each 1 … " + std::to_string(RT_VOLUME_MAX_N) +
                          ") and then exactly nx*ny*nz little-endian float32 densities, finite and not negative: " + grid_file;
        }
        // --fog-heat FILE (with --fog-glow and --fog-grid, checked above): the grid the emission follows, of the density grid's dimensions
        if (fog_bad.empty() && fog_glow_on && fog_glow.source == 2) {
            if (!read_grid_file(fog_heat_file, fog_heat_n, fog_heat))
                fog_bad = "--fog-heat takes a FILE of --fog-grid's format, finite and not negative: " + fog_heat_file;
            else if (fog_heat_n[0] != fog_n[0] || fog_heat_n[1] != fog_n[1] || fog_heat_n[2] != fog_n[2])
                fog_bad = "--fog-heat: the heat grid's dimensions differ from the density grid's: " + fog_heat_file;
        }
        if (fog_bad.empty() && fog_glow_on && !(fog.sigma_t > 0.0f) && (fog_glow.radiance[0] > 0.0f || fog_glow.radiance[1] > 0.0f || fog_glow.radiance[2] > 0.0f))
            fog_bad = "--fog-glow needs --fog SIGMA with SIGMA > 0: a glow without extinction has no kernel";
        if (!fog_bad.empty()) {
            std::cerr << "rtp_main: " << fog_bad << "\n";
            return 99;
        }
    }
    // extension: `--glossy`, with `--nee`, with `--env` in mode mis or light, or with `--lit`, and only with them: METAL's reflect branch
    // takes light samples too (rt_nee_params.glossy / rt_env_params.glossy = 1) — the switch of every light that is on.
    bool glossy_on = false;
    {
        bool sampled = lit_on;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--glossy") glossy_on = true;
            if (arg == "--nee") sampled = true;
        }
        if (glossy_on && !sampled) {
            bool env_flag = false, env_path = false;
            for (int a = 2; a < argc; ++a) {
                const std::string arg = argv[a];
                if (arg == "--env") env_flag = true;
                if (arg == "--env-mode" && a + 1 < argc && std::string(argv[a + 1]) == "path") env_path = true;
            }
            sampled = env_flag && !env_path;
        }
        if (glossy_on && !sampled) {
            std::cerr << "rtp_main: --glossy takes light samples at METAL's reflect branch: it needs --nee, --env (mode mis or light) or --lit\n";
            return 99;
        }
        if (glossy_on) lit_nee.glossy = 1;
    }
    // extension: `--gpu --env FILE[:N] [--env-mode path|mis|light] [--env-scale S] [--env-up y|z]`: every frame through rt_render_env on one
    // GPU, lit by the lat-long image FILE (PFM or Radiance .hdr) resampled into an N x N octahedral map (N defaults to 1024); mis is the
    // default mode, --env-up z turns the map for a z-up scene such as the default configuration; the same saver bytes, --aov /
    // --denoise as with --nee.  Not with --nee, --lens, --motion-blur, --adaptive, --denoise-temporal, --devices, --shard or RTP_DEVICES.
    {
        bool env_on = false, env_others = getenv("RTP_DEVICES") != nullptr;
        std::string env_bad, env_file;
        int env_n = 1024;
        rt_env_params ep;
        rt_env_params_init(&ep);
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            const std::string value = a + 1 < argc ? argv[a + 1] : "";
            if (!lit_on && (arg == "--nee" || arg == "--lens" || arg == "--motion-blur" || arg == "--adaptive" || arg == "--denoise-temporal" ||
                            arg == "--devices" || arg == "--shard"))
                env_others = true;
            if (arg == "--env") {
                env_on = true;
                env_file = value;
                const size_t colon = env_file.rfind(':');
                if (colon != std::string::npos && colon + 1 < env_file.size() && env_file.find_first_not_of("0123456789", colon + 1) == std::string::npos) {
                    env_n = env_file.size() - colon - 1 > 5 ? 0 : atoi(env_file.c_str() + colon + 1);
                    env_file.erase(colon);
                }
                if (env_file.empty()) env_bad = "--env takes FILE[:N]";
                else if (env_n < 1 || env_n > RT_ENV_MAX_N) env_bad = "--env FILE:N takes N from 1 to " + std::to_string(RT_ENV_MAX_N);
            } else if (arg == "--env-mode") {
                if (value == "path") ep.mode = 0;
                else if (value == "mis") ep.mode = 1;
                else if (value == "light") ep.mode = 2;
                else env_bad = "--env-mode takes path, mis (default) or light";
            } else if (arg == "--env-scale") {
                char *end = nullptr;
                ep.scale = strtof(value.c_str(), &end);
                if (value.empty() || *end != 0 || !(std::isfinite(ep.scale) && ep.scale >= 0.0f)) env_bad = "--env-scale takes a finite number that is not negative";
            } else if (arg == "--env-up") {
                if (value == "z") {
                    const float z_up[9] = {1, 0, 0, 0, 0, 1, 0, -1, 0};        // environment y = world z
                    for (int k = 0; k < 9; ++k) ep.rot[k] = z_up[k];
                } else if (value != "y") {
                    env_bad = "--env-up takes y (default) or z";
                }
            }
        }
        if (glossy_on && ep.mode != 0) ep.glossy = 1;
        if (!env_on)
            for (int a = 2; a < argc; ++a)
                if (std::string(argv[a]).compare(0, 6, "--env-") == 0) env_bad = std::string(argv[a]) + " needs --env FILE";
        if (env_on || !env_bad.empty()) {
            if (!env_bad.empty()) {
                std::cerr << "rtp_main: " << env_bad << "\n";
                return 99;
            }
            if (env_others) {
                std::cerr << "rtp_main: --env renders frame after frame on one GPU: it cannot be combined with --nee, --lens, --motion-blur, "
                             "--adaptive, --denoise-temporal, --devices, --shard or RTP_DEVICES\n";
                return 99;
            }
            rtp::HdrImage image;
            std::string error;
            if (!rtp::load_hdr_image(env_file, image, error)) {
                std::cerr << "rtp_main: --env: " << error << "\n";
                return 99;
            }
            std::vector<float> map(static_cast<size_t>(env_n) * env_n * 3);
            rt_env *env = nullptr;
            if (rt_env_from_equirect(image.rgb.data(), image.width, image.height, env_n, map.data()) != RT_OK ||
                rt_env_create(map.data(), env_n, &env) != RT_OK) {
                std::cerr << "rtp_main: --env: " << env_file << ": " << rt_get_last_error_string() << "\n";
                return 99;
            }
            if (lit_on) {
                lit_env = env;
                lit_ep = ep;
            } else {
                rt_lens_params pinhole;
                rt_lens_params_init(&pinhole);
                rtp::gpu_render_lens(params, desc, pinhole, 0.0f, aov, denoise, nullptr, env, &ep);
                rt_env_destroy(env);
                return 0;
            }
        }
    }
    // extension: `--gpu --nee [mis|light]`: every frame through rt_render_nee on one GPU (direct light sampling of the emissive spheres,
    // combined with the path's own sample by the power heuristic, or alone), the same saver bytes; --aov / --denoise as without it
    // (first-hit AOVs do not depend on the estimator).  Not with --lens, --motion-blur, --adaptive, --denoise-temporal, --devices,
    // --shard or RTP_DEVICES.  `--light-tree` (with --nee, or with --lit, whose emitters are sampled): the emitter of a light sample is
    // picked by the light tree, by where the shaded point is (rt_nee_params.select = 1), instead of the power table.
    {
        bool nee_on = false, nee_bad = false, tree_on = false, nee_others = getenv("RTP_DEVICES") != nullptr;
        rt_nee_params nee;
        rt_nee_params_init(&nee);
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--lens" || arg == "--motion-blur" || arg == "--adaptive" || arg == "--denoise-temporal" || arg == "--devices" ||
                arg == "--shard")
                nee_others = true;
            if (arg == "--light-tree") tree_on = true;
            if (arg == "--nee") {
                nee_on = true;
                if (a + 1 < argc && argv[a + 1][0] != '-') {
                    const std::string mode = argv[a + 1];
                    if (mode == "mis") nee.mis = 1;
                    else if (mode == "light") nee.mis = 0;
                    else nee_bad = true;
                }
            }
        }
        if (tree_on && !nee_on && !lit_on) {
            std::cerr << "rtp_main: --light-tree picks the emitter of a light sample: it needs --nee or --lit\n";
            return 99;
        }
        if (tree_on) {
            nee.select = 1;
            lit_nee.select = 1;
        }
        if (glossy_on) nee.glossy = 1;
        if (nee_on) {
            if (nee_bad) {
                std::cerr << "rtp_main: --nee takes mis (default) or light\n";
                return 99;
            }
            if (lit_on) {
                lit_nee = nee;
            } else if (nee_others) {
                std::cerr << "rtp_main: --nee renders frame after frame on one GPU: it cannot be combined with --lens, --motion-blur, "
                             "--adaptive, --denoise-temporal, --devices, --shard or RTP_DEVICES\n";
                return 99;
            }
            if (!lit_on) {
                rt_lens_params pinhole;
                rt_lens_params_init(&pinhole);
                rtp::gpu_render_lens(params, desc, pinhole, 0.0f, aov, denoise, &nee);
                return 0;
            }
        }
    }
    // extension: `--gpu --lens R:F` (thin lens of radius R focused at distance F) and / or `--gpu --motion-blur S` (shutter open from
    // frame n to n + S, 0 < S <= 1): every frame through rt_render_lens on one GPU, the same saver bytes (--aov / --denoise from
    // rt_render_aov_lens).  The temporal filter's reprojection assumes a pinhole: not with --denoise-temporal; nor with --adaptive,
    // --devices, --shard or RTP_DEVICES.
    {
        bool lens_on = false, motion_on = false, lens_bad = false;
        rt_lens_params lens;
        rt_lens_params_init(&lens);
        float shutter = 0.0f;
        bool others = getenv("RTP_DEVICES") != nullptr;
        for (int a = 2; a < argc; ++a) {
            const std::string arg = argv[a];
            if (arg == "--denoise-temporal" || arg == "--adaptive" || arg == "--devices" || arg == "--shard") others = true;
            if (arg == "--lens") {
                lens_on = true;
                float r = 0, f = 0;
                char tail = 0;
                if (a + 1 >= argc || sscanf(argv[a + 1], "%f:%f%c", &r, &f, &tail) != 2 || !(r >= 0.0f) || !(f > 0.0f) || !std::isfinite(r) ||
                    !std::isfinite(f))
                    lens_bad = true;
                lens.lens_radius = r;
                lens.focus_distance = f;
            }
            if (arg == "--motion-blur") {
                motion_on = true;
                char tail = 0;
                if (a + 1 >= argc || sscanf(argv[a + 1], "%f%c", &shutter, &tail) != 1 || !(shutter > 0.0f && shutter <= 1.0f)) lens_bad = true;
            }
        }
        if (lens_on || motion_on || lit_on) {
            if (lens_bad) {
                std::cerr << "rtp_main: --lens takes R:F (R >= 0, F > 0, finite) and --motion-blur takes S (0 < S <= 1)\n";
                return 99;
            }
            if (others) {
                std::cerr << "rtp_main: --lens / --motion-blur render frame after frame on one GPU: they cannot be combined with "
                             "--denoise-temporal, --adaptive, --devices, --shard or RTP_DEVICES\n";
                return 99;
            }
            if (lit_on) {
                rt_lit_params lit;
                rt_lit_params_init(&lit);
                lit.nee = &lit_nee;
                lit.env = lit_env;
                lit.env_params = &lit_ep;
                rt_volume *fog_volume = nullptr;
                if (!fog_grid.empty() && rt_volume_create(fog_grid.data(), fog_n[0], fog_n[1], fog_n[2], &fog_volume) != RT_OK) {
                    std::cerr << "rtp_main: --fog-grid: " << rt_get_last_error_string() << "\n";
                    return 99;
                }
                rt_volume *fog_heat_volume = nullptr;
                if (!fog_heat.empty() && rt_volume_create(fog_heat.data(), fog_heat_n[0], fog_heat_n[1], fog_heat_n[2], &fog_heat_volume) != RT_OK) {
                    std::cerr << "rtp_main: --fog-heat: " << rt_get_last_error_string() << "\n";
                    return 99;
                }
                rt_glow_sampler *fog_sampler = nullptr;
                if (fog_glow_sample_on && rt_glow_sampler_create(fog_volume, fog_glow.source, fog_heat_volume, &fog_sampler) != RT_OK) {
                    std::cerr << "rtp_main: --fog-glow-sample: " << rt_get_last_error_string() << "\n";
                    return 99;
                }
                rtp::gpu_render_lens(params, desc, lens, shutter, aov, denoise, nullptr, nullptr, nullptr, &lit, fog_noise_on ? &fog_noise : noise_on ? &noise : nullptr,
                                     denoise_adaptive, &stop_rule, denoise_adaptive_temporal, fog_on ? &fog : nullptr, stop_history, fog_volume, fog_denoise,
                                     fog_tint_on ? &fog_tint : nullptr, fog_glow_on ? &fog_glow : nullptr, fog_heat_volume,
                                     fog_glow_sample_on ? &fog_glow_sample : nullptr, fog_sampler);
                rt_glow_sampler_destroy(fog_sampler);
                rt_volume_destroy(fog_heat_volume);
                rt_volume_destroy(fog_volume);
                rt_env_destroy(lit_env);
                return 0;
            }
            rtp::gpu_render_lens(params, desc, lens, shutter, aov, denoise);
            return 0;
        }
    }
    if (denoise && temporal) {
        std::cerr << "rtp_main: --denoise and --denoise-temporal both write <frame>.denoised: choose one\n";
        return 2;
    }
    // extension: `--gpu --devices N` (or RTP_DEVICES=N) renders the animation with the pipelined
    // multi-GPU driver; the default is the reference's frame-after-frame loop.
    int devices = 0;
    if (const char *env = getenv("RTP_DEVICES")) devices = atoi(env);
    for (int a = 2; a + 1 < argc; ++a)
        if (std::string(argv[a]) == "--devices") devices = atoi(argv[a + 1]);
    if (aov || denoise || temporal) {
        for (int a = 2; a < argc; ++a)
            if (std::string(argv[a]) == "--devices" || std::string(argv[a]) == "--shard") devices = 1;
        if (devices > 0) {
            std::cerr << "rtp_main: " << (aov ? "--aov" : denoise ? "--denoise" : "--denoise-temporal")
                      << " renders frame after frame on one GPU: it cannot be combined with --devices, --shard or RTP_DEVICES\n";
            return 2;
        }
    }
    // extension: `--gpu --adaptive <threshold> [--adaptive-spp min:batch:max]` renders every frame with per-pixel adaptive sampling
    // (rt_render_adaptive; default 16:16:256) and saves it through rt_tonemap_spp — one GPU, frame after frame
    for (int a = 2; a + 1 < argc; ++a)
        if (std::string(argv[a]) == "--adaptive") {
            rt_adaptive_params ap;
            rt_adaptive_params_init(&ap);
            ap.threshold = strtof(argv[a + 1], nullptr);
            for (int b = 2; b + 1 < argc; ++b)
                if (std::string(argv[b]) == "--adaptive-spp" &&
                    sscanf(argv[b + 1], "%d:%d:%d", &ap.min_spp, &ap.batch_spp, &ap.max_spp) != 3) {
                    std::cerr << "rtp_main: --adaptive-spp takes min:batch:max\n";
                    return 2;
                }
            if (aov || denoise || temporal || devices > 0) {
                std::cerr << "rtp_main: --adaptive renders frame after frame on one GPU: it cannot be combined with --aov, --denoise, "
                             "--denoise-temporal, --devices, --shard or RTP_DEVICES\n";
                return 2;
            }
            for (int b = 2; b < argc; ++b)
                if (std::string(argv[b]) == "--shard") {
                    std::cerr << "rtp_main: --adaptive cannot be combined with --shard\n";
                    return 2;
                }
            rtp::gpu_render_adaptive(params, desc, ap, denoise_adaptive, &stop_rule, denoise_adaptive_temporal, stop_history);
            return 0;
        }
    // extension: `--gpu --shard N` splits EVERY frame over N GPUs (0 = all of the node) with one RCCL gather per frame
    for (int a = 2; a + 1 < argc; ++a)
        if (std::string(argv[a]) == "--shard") {
            rtp::gpu_render_sharded(params, desc, atoi(argv[a + 1]));
            return 0;
        }
    if (devices > 0) {
        rtp::gpu_render_pipelined(params, desc, devices);
        return 0;
    }
    rt_scene *scene = nullptr;
    RTP_CHECK(rt_scene_create(&desc, &scene));
    rtp::bind_scene(scene);
    rtp::gpu_render(params, aov, denoise, temporal);
    RTP_CHECK(rt_scene_destroy(scene));
    return 0;
}
