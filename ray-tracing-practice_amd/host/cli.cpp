// cli.cpp — parse_cli (cli.h): one pass over argv that reads every flag's value, then one ordered list of refusals.  The order
// of that list is the behaviour: the first refusal that applies is the one reported, and the lines marked "oddity" are orders and rules one
// would not guess, which tests/golden/cli_record.json pins.  Of rtp_amd.h only the two size limits are used: nothing here calls the render
// library.
#include "cli.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>

#include "../../include/rtp_amd.h"

namespace rtp {
namespace {

// A grid file of --fog-grid and --fog-heat: the ASCII header "VOL1\nnx ny nz\n" and then exactly nx * ny * nz little-endian float32 (this
// build's hosts are little-endian, like the file), finite and not negative, x fastest
bool read_grid_file(const std::string &file, CliGrid &grid) {
    FILE *f = file.empty() ? nullptr : fopen(file.c_str(), "rb");
    char magic[8] = {0}, eol = 0;
    size_t count = 0;
    int *n = grid.n;
    bool ok = f && fgets(magic, sizeof(magic), f) && std::strcmp(magic, "VOL1\n") == 0 && fscanf(f, "%d %d %d%c", &n[0], &n[1], &n[2], &eol) == 4 && eol == '\n';
    for (int k = 0; ok && k < 3; ++k) ok = n[k] >= 1 && n[k] <= RT_VOLUME_MAX_N;
    if (ok) {
        count = static_cast<size_t>(n[0]) * n[1] * n[2];
        grid.cells.resize(count);
        ok = fread(grid.cells.data(), sizeof(float), count, f) == count && fgetc(f) == EOF;
    }
    for (size_t k = 0; ok && k < count; ++k) ok = std::isfinite(grid.cells[k]) && grid.cells[k] >= 0.0f;
    if (f) fclose(f);
    return ok;
}

bool spp_in_range(const CliSpp &s) { return s.min_spp >= 2 && s.batch_spp >= 1 && s.max_spp >= s.min_spp && s.max_spp <= 65536; }

bool three_not_negative(const std::string &value, float out[3]) {
    char tail = 0;
    bool ok = sscanf(value.c_str(), "%f,%f,%f%c", &out[0], &out[1], &out[2], &tail) == 3;
    for (int k = 0; ok && k < 3; ++k) ok = std::isfinite(out[k]) && out[k] >= 0.0f;
    return ok;
}

bool threshold_alone(const std::string &value, float &out) {
    char *end = nullptr;
    out = strtof(value.c_str(), &end);
    return !value.empty() && *end == 0 && std::isfinite(out) && out >= 0.0f;
}

// What the pass keeps beside the values in Cli: where each element stood last, and per group of flags that are judged together the text of
// the group's last faulty value in argv order (oddity: a later good value of the same flag does not clear it)
struct Pass {
    std::map<std::string, int> at;          // element → its last index; "--denoise*": the last element that begins with --denoise
    std::string denoise_word, env_dash_word;          // that element; the last element that begins with --env-
    std::string fog_word;                             // the last element that begins with --fog
    std::string glow_bad, tint_bad, fog_noise_bad, fog_adaptive_bad, noise_bad, fog_bad, env_bad;
    bool nee_bad = false, lens_bad = false, adaptive_spp_bad = false;
    bool glow_by_density = false, adaptive_valued = false, shard_valued = false;
    bool env_mode_path = false;          // some --env-mode says path (for --glossy: any of them counts, not the last)
    std::string stop_word, grid_file, heat_file;

    bool has(const char *flag) const { return at.count(flag) != 0; }
    bool any(std::initializer_list<const char *> flags) const {
        for (const char *f : flags)
            if (has(f)) return true;
        return false;
    }
    // the one of these that stands last in argv ("" when none does)
    std::string last_of(std::initializer_list<const char *> flags) const {
        int best = -1;
        std::string word;
        for (const char *f : flags) {
            const auto it = at.find(f);
            if (it == at.end() || it->second < best) continue;
            best = it->second;
            word = std::strcmp(f, "--denoise*") == 0 ? denoise_word : std::string(f);
        }
        return word;
    }
};

// The one pass: every element from argv[2] on is looked at as a flag, the element after it as its value ("" at the end) — also an element
// that served as the value of the one before (`--env --lit` means file --lit and --lit on)
void read_values(int argc, const char *const *argv, const char *rtp_devices, Cli &cli, Pass &p) {
    if (rtp_devices) cli.devices = atoi(rtp_devices);
    for (int a = 2; a < argc; ++a) {
        const std::string arg = argv[a];
        const bool valued = a + 1 < argc;
        const std::string value = valued ? argv[a + 1] : "";
        char tail = 0;
        p.at[arg] = a;
        if (arg.compare(0, 9, "--denoise") == 0) {
            p.at["--denoise*"] = a;
            p.denoise_word = arg;
        }
        if (arg.compare(0, 6, "--env-") == 0) p.env_dash_word = arg;
        if (arg.compare(0, 5, "--fog") == 0) p.fog_word = arg;
        if (arg == "--stop-rule") p.stop_word = value;
        if (arg == "--fog-grid") p.grid_file = value;
        if (arg == "--fog-heat") p.heat_file = value;
        if (arg == "--fog-glow-sample") {
            if (value != "mis" && value != "light") p.glow_bad = "--fog-glow-sample takes mis or light";
            cli.fog_glow_sample_mis = value == "light" ? 0 : 1;
        }
        if (arg == "--fog-glow") {
            std::string rgb = value;
            const std::string suffix = ":density";
            p.glow_by_density = rgb.size() > suffix.size() && rgb.compare(rgb.size() - suffix.size(), suffix.size(), suffix) == 0;
            if (p.glow_by_density) rgb.resize(rgb.size() - suffix.size());
            if (!three_not_negative(rgb, cli.fog_glow_radiance)) p.glow_bad = "--fog-glow takes R,G,B[:density]: three finite numbers, none negative";
        }
        if (arg == "--fog-tint" && !three_not_negative(value, cli.fog_tint_rgb)) p.tint_bad = "--fog-tint takes R,G,B: three finite numbers, none negative";
        if (arg == "--fog-noise-target" || arg == "--fog-adaptive") {          // one value grammar for both
            const bool rungs = arg == "--fog-adaptive";
            float &threshold = rungs ? cli.fog_adaptive_threshold : cli.fog_noise_threshold;
            char *end = nullptr;
            threshold = strtof(value.c_str(), &end);
            bool ok = end != value.c_str() && std::isfinite(threshold) && threshold >= 0.0f;
            if (ok && *end == ':') {
                CliSpp &s = rungs ? cli.fog_adaptive_spp : cli.fog_noise_spp;
                s.given = true;
                ok = sscanf(end + 1, "%d:%d:%d%c", &s.min_spp, &s.batch_spp, &s.max_spp, &tail) == 3 && spp_in_range(s);
            } else if (ok) {
                ok = *end == 0;
            }
            if (!ok) (rungs ? p.fog_adaptive_bad : p.fog_noise_bad) = arg + " takes T[:min:batch:max] with T finite and not negative, min >= 2, batch >= 1 and min <= max <= 65536";
        }
        if (arg == "--noise-target" && !threshold_alone(value, cli.noise_threshold)) p.noise_bad = "--noise-target takes a finite threshold that is not negative";
        if (arg == "--noise-spp") {
            CliSpp &s = cli.noise_spp;
            s.given = true;
            if (sscanf(value.c_str(), "%d:%d:%d%c", &s.min_spp, &s.batch_spp, &s.max_spp, &tail) != 3 || !spp_in_range(s))
                p.noise_bad = "--noise-spp takes min:batch:max with min >= 2, batch >= 1 and min <= max <= 65536";
        }
        if (arg == "--fog") {
            cli.fog_albedo = 1.0f;
            cli.fog_g = 0.0f;
            // one to three numbers between colons, each read to its end
            float *into[3] = {&cli.fog_sigma, &cli.fog_albedo, &cli.fog_g};
            bool ok = !value.empty();
            const char *at = value.c_str();
            for (int got = 0; ok; ++got) {
                char *end = nullptr;
                if (got == 3) { ok = false; break; }
                *into[got] = strtof(at, &end);
                ok = end != at && (*end == 0 || *end == ':');
                if (!ok || *end == 0) break;
                at = end + 1;
            }
            if (!ok || !(std::isfinite(cli.fog_sigma) && cli.fog_sigma >= 0.0f) || !(cli.fog_albedo >= 0.0f && cli.fog_albedo <= 1.0f) || !(std::fabs(cli.fog_g) <= 0.95f))
                p.fog_bad = "--fog takes SIGMA[:ALBEDO[:G]] with SIGMA >= 0 and finite, 0 <= ALBEDO <= 1 and |G| <= 0.95";
        }
        if (arg == "--fog-ball") {
            cli.fog_region = 1;
            float *c = cli.fog_a, &r = cli.fog_b[0];
            if (sscanf(value.c_str(), "%f,%f,%f,%f%c", &c[0], &c[1], &c[2], &r, &tail) != 4 || !(r > 0.0f) || !std::isfinite(r) || !std::isfinite(c[0]) ||
                !std::isfinite(c[1]) || !std::isfinite(c[2]))
                p.fog_bad = "--fog-ball takes cx,cy,cz,r with finite numbers and r > 0";
        }
        if (arg == "--fog-box") {
            cli.fog_region = 2;
            float *lo = cli.fog_a, *hi = cli.fog_b;
            bool ok = sscanf(value.c_str(), "%f,%f,%f,%f,%f,%f%c", &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2], &tail) == 6;
            for (int k = 0; ok && k < 3; ++k) ok = std::isfinite(lo[k]) && std::isfinite(hi[k]) && lo[k] < hi[k];
            if (!ok) p.fog_bad = "--fog-box takes x0,y0,z0,x1,y1,z1 with finite numbers and x0 < x1, y0 < y1, z0 < z1";
        }
        if (arg == "--env") {
            cli.env_file = value;
            const size_t colon = cli.env_file.rfind(':');
            if (colon != std::string::npos && colon + 1 < cli.env_file.size() && cli.env_file.find_first_not_of("0123456789", colon + 1) == std::string::npos) {
                cli.env_n = cli.env_file.size() - colon - 1 > 5 ? 0 : atoi(cli.env_file.c_str() + colon + 1);          // oddity: an N stays for a later --env without one
                cli.env_file.erase(colon);
            }
            if (cli.env_file.empty()) p.env_bad = "--env takes FILE[:N]";
            else if (cli.env_n < 1 || cli.env_n > RT_ENV_MAX_N) p.env_bad = "--env FILE:N takes N from 1 to " + std::to_string(RT_ENV_MAX_N);
        }
        if (arg == "--env-mode") {
            if (value == "path") cli.env_mode = 0, p.env_mode_path = true;
            else if (value == "mis") cli.env_mode = 1;
            else if (value == "light") cli.env_mode = 2;
            else p.env_bad = "--env-mode takes path, mis (default) or light";
        }
        if (arg == "--env-scale") {
            cli.env_scale_given = true;
            if (!threshold_alone(value, cli.env_scale)) p.env_bad = "--env-scale takes a finite number that is not negative";
        }
        if (arg == "--env-up") {
            if (value == "z") cli.env_up_z = true;          // oddity: a later --env-up y does not turn the map back
            else if (value != "y") p.env_bad = "--env-up takes y (default) or z";
        }
        if (arg == "--nee" && valued && (value.empty() || value[0] != '-')) {          // a word after --nee is its mode unless it is a flag
            if (value == "mis") cli.nee_mis = 1;
            else if (value == "light") cli.nee_mis = 0;
            else p.nee_bad = true;
        }
        if (arg == "--lens") {
            float r = 0, f = 0;
            if (sscanf(value.c_str(), "%f:%f%c", &r, &f, &tail) != 2 || !(r >= 0.0f) || !(f > 0.0f) || !std::isfinite(r) || !std::isfinite(f)) p.lens_bad = true;
            cli.lens_radius = r;
            cli.lens_focus = f;
        }
        if (arg == "--motion-blur" && (sscanf(value.c_str(), "%f%c", &cli.shutter, &tail) != 1 || !(cli.shutter > 0.0f && cli.shutter <= 1.0f))) p.lens_bad = true;
        // oddity: --devices, --adaptive, --adaptive-spp and --shard as the last element carry no value and select no driver, but count as given
        if (arg == "--devices" && valued) cli.devices = atoi(value.c_str());
        if (arg == "--adaptive" && valued && !p.adaptive_valued) {          // the first one with a value
            p.adaptive_valued = true;
            cli.adaptive_threshold = strtof(value.c_str(), nullptr);
        }
        if (arg == "--adaptive-spp" && valued) {          // (no check of range or tail: rt_render_adaptive refuses a bad triple)
            CliSpp &s = cli.adaptive_spp;
            s.given = true;
            if (sscanf(value.c_str(), "%d:%d:%d", &s.min_spp, &s.batch_spp, &s.max_spp) != 3) p.adaptive_spp_bad = true;
        }
        if (arg == "--shard" && valued && !p.shard_valued) {
            p.shard_valued = true;
            cli.shards = atoi(value.c_str());
        }
    }
    cli.aov = p.has("--aov");
    cli.denoise = p.has("--denoise");
    cli.denoise_temporal = p.has("--denoise-temporal");
    cli.denoise_adaptive = p.has("--denoise-adaptive");
    cli.denoise_adaptive_temporal = p.has("--denoise-adaptive-temporal");
    cli.stop_history = p.has("--stop-history");
    cli.lit = p.has("--lit");
    cli.glossy = p.has("--glossy");
    cli.light_tree = p.has("--light-tree");
    cli.nee = p.has("--nee");
    cli.env = p.has("--env");
    cli.fog = p.has("--fog");
    cli.fog_denoise = p.has("--fog-denoise");
    cli.fog_tint = p.has("--fog-tint");
    cli.fog_glow = p.has("--fog-glow");
    cli.fog_glow_sample = p.has("--fog-glow-sample");
    cli.fog_noise = p.has("--fog-noise-target");
    cli.fog_adaptive = p.has("--fog-adaptive");
    cli.noise = p.has("--noise-target");
    cli.lens = p.has("--lens");
    cli.motion_blur = p.has("--motion-blur");
    cli.split = p.has("--split");
    cli.stop_rule = p.stop_word == "near" ? 1 : 0;
    cli.fog_glow_source = p.has("--fog-heat") ? 2 : (p.glow_by_density ? 1 : 0);
}

}  // namespace

bool parse_cli(int argc, const char *const *argv, const char *rtp_devices, Cli &cli, CliRefusal &refusal) {
    Pass p;
    read_values(argc, argv, rtp_devices, cli, p);
    const Cli &c = cli;
    auto refuse = [&refusal](int code, const std::string &text) {
        refusal.code = code;
        refusal.text = text;
        return false;
    };
    auto accept = [&cli](Cli::Driver driver) {
        cli.driver = driver;
        return true;
    };
    const bool grid = p.has("--fog-grid"), heat = p.has("--fog-heat"), ball = p.has("--fog-ball"), box = p.has("--fog-box");
    const bool adaptive = p.has("--adaptive"), many = p.any({"--devices", "--shard"}), env_devices = rtp_devices != nullptr;
    const bool adaptive_frames = adaptive || (c.lit && c.noise);          // what --denoise-adaptive*, --stop-rule filter or steer
    std::string other;

    // ---- the refusals, in order: the first that applies is the answer ----
    // --split (first, so that every refusal of a command line with it names it)
    if (c.split && !c.lit) return refuse(99, "--split writes the direct and the indirect light of --lit frames: it needs --lit");
    if (c.split && !p.fog_word.empty()) return refuse(99, "--split cannot be combined with " + p.fog_word + ": the fog calls have no split");
    other = p.last_of({"--noise-target", "--noise-spp", "--adaptive", "--adaptive-spp", "--devices", "--shard", "--denoise-temporal", "--denoise-adaptive",
                       "--denoise-adaptive-temporal", "--stop-rule", "--stop-history"});
    if (c.split && (!other.empty() || env_devices))
        return refuse(99, "--split cannot be combined with " + (other.empty() ? std::string("RTP_DEVICES") : other) +
                              " (not with --noise-target, --adaptive, --devices, --shard, RTP_DEVICES or the temporal and adaptive denoise flags)");
    // --fog-denoise (before the flags it excludes, so that the refusal names it)
    if (c.fog_denoise && !c.fog) return refuse(99, "--fog-denoise filters fogged frames: it needs --lit --fog SIGMA");
    other = p.last_of({"--denoise*", "--aov", "--adaptive", "--devices", "--shard"});
    if (c.fog_denoise && !other.empty())
        return refuse(99, "--fog-denoise cannot be combined with " + other + " (not with --denoise*, --aov, --adaptive, --devices or --shard)");
    // --fog-glow, --fog-heat, --fog-glow-sample: a faulty value first
    if (!p.glow_bad.empty()) return refuse(99, p.glow_bad);
    if (heat && !c.fog_glow) return refuse(99, "--fog-heat shapes the emission of --fog-glow: it needs --fog-glow R,G,B");
    if (c.fog_glow && !c.fog) return refuse(99, "--fog-glow makes the medium of --fog emit: it needs --lit --fog SIGMA with SIGMA > 0");
    other = p.last_of({"--fog-tint", "--fog-noise-target", "--fog-denoise"});
    if (c.fog_glow && !other.empty()) return refuse(99, "--fog-glow cannot be combined with " + other + ": the chroma, adaptive, AOV and denoise calls take no glow");
    if (c.fog_glow && heat && p.glow_by_density) return refuse(99, "--fog-glow R,G,B:density and --fog-heat exclude each other: the emission follows one grid");
    if (c.fog_glow && p.glow_by_density && !grid) return refuse(99, "--fog-glow R,G,B:density follows the density grid: it needs --fog-grid FILE");
    if (c.fog_glow && heat && !grid) return refuse(99, "--fog-heat has the dimensions of the density grid: it needs --fog-grid FILE");
    if (c.fog_glow_sample && !c.fog_glow) return refuse(99, "--fog-glow-sample aims at the glow: it needs --fog-glow R,G,B");
    if (c.fog_glow_sample && !grid)
        return refuse(99, "--fog-glow-sample picks a cell of the density grid: it needs --fog-grid FILE (a homogeneous box can pass a 1 x 1 x 1 grid)");
    // --fog-tint
    if (!p.tint_bad.empty()) return refuse(99, p.tint_bad);
    if (c.fog_tint && !c.fog) return refuse(99, "--fog-tint colours the extinction of --fog: it needs --lit --fog SIGMA");
    other = p.last_of({"--fog-noise-target", "--fog-denoise"});
    if (c.fog_tint && !other.empty()) return refuse(99, "--fog-tint cannot be combined with " + other + ": the adaptive, AOV and denoise calls take no tint (grey fog only)");
    // --fog-noise-target
    if (!p.fog_noise_bad.empty()) return refuse(99, p.fog_noise_bad);
    if (c.fog_noise && !c.fog) return refuse(99, "--fog-noise-target sets the noise target of fogged frames: it needs --lit --fog SIGMA");
    other = p.last_of({"--adaptive", "--denoise*", "--aov", "--stop-rule", "--stop-history", "--noise-target"});
    if (c.fog_noise && !other.empty())
        return refuse(99, "--fog-noise-target cannot be combined with " + other + " (not with --adaptive, --denoise*, --aov, --stop-rule, --stop-history or --noise-target)");
    // --fog-adaptive (behind --fog-noise-target's block: what that flag refuses, it refuses under its own name)
    if (!p.fog_adaptive_bad.empty()) return refuse(99, p.fog_adaptive_bad);
    if (c.fog_adaptive && !(c.fog && c.lit)) return refuse(99, "--fog-adaptive sets the noise target of fogged frames, tinted and glowing ones too: it needs --lit --fog SIGMA");
    other = p.last_of({"--fog-noise-target", "--fog-denoise", "--adaptive", "--denoise*", "--aov", "--stop-rule", "--stop-history", "--noise-target"});
    if (c.fog_adaptive && !other.empty())
        return refuse(99, "--fog-adaptive cannot be combined with " + other +
                              " (not with --fog-noise-target, --fog-denoise, --adaptive, --denoise*, --aov, --stop-rule, --stop-history or --noise-target)");
    // --denoise-adaptive-temporal, --stop-history, --denoise-adaptive, --stop-rule: exit code 2
    if (c.denoise_adaptive_temporal && (c.denoise || c.denoise_temporal || c.aov || env_devices || many || p.any({"--denoise-adaptive", "--lens", "--motion-blur"})))
        return refuse(2, "--denoise-adaptive-temporal writes <frame>.denoised from pinhole frames and AOVs of its own on one GPU: it cannot "
                         "be combined with --denoise, --denoise-temporal, --denoise-adaptive, --aov, --lens, --motion-blur, --devices, --shard or "
                         "RTP_DEVICES");
    if (c.denoise_adaptive_temporal && !adaptive_frames)
        return refuse(2, "--denoise-adaptive-temporal filters adaptively sampled frames: it needs --adaptive T or --lit --noise-target T");
    if (c.stop_history && !c.denoise_adaptive_temporal)
        return refuse(2, "--stop-history feeds the history of --denoise-adaptive-temporal back into the stopping rule: it needs that flag");
    if (c.denoise_adaptive && (c.denoise || c.denoise_temporal || c.aov))
        return refuse(2, "--denoise-adaptive writes <frame>.denoised from AOVs of its own: it cannot be combined with --denoise, "
                         "--denoise-temporal or --aov");
    if (c.denoise_adaptive && !adaptive_frames) return refuse(2, "--denoise-adaptive filters adaptively sampled frames: it needs --adaptive T or --lit --noise-target T");
    if (p.has("--stop-rule") && p.stop_word != "own" && p.stop_word != "near") return refuse(2, "--stop-rule takes own or near");          // the last one's word
    if (p.has("--stop-rule") && !adaptive_frames)
        return refuse(2, "--stop-rule picks the stopping rule of adaptively sampled frames: it needs --adaptive T or --lit --noise-target T");
    // --noise-target, --noise-spp.  oddity: a missing --noise-target or --lit outranks a faulty value here; the third line does not
    if (c.noise_spp.given && !c.noise) return refuse(99, "--noise-spp needs --noise-target T");
    if (c.noise && !c.lit) return refuse(99, "--noise-target sets the noise target of --lit frames: it needs --lit");
    if (!p.noise_bad.empty()) return refuse(99, p.noise_bad);
    if (c.noise && (adaptive || c.aov || c.denoise)) return refuse(99, "--noise-target cannot be combined with --adaptive, --denoise or --aov");
    // --lit
    if (c.lit && (env_devices || adaptive || c.denoise_temporal || many))
        return refuse(99, "--lit renders frame after frame on one GPU: it cannot be combined with --adaptive, --denoise-temporal, "
                          "--devices, --shard or RTP_DEVICES");
    // --fog, --fog-ball, --fog-box, --fog-grid.  oddity: each of these six outranks a faulty value of the three flags
    if ((ball || box) && !c.fog) return refuse(99, "--fog-ball and --fog-box bound the medium of --fog: they need --fog SIGMA");
    if (ball && box) return refuse(99, "--fog-ball and --fog-box exclude each other: the medium has one region");
    if (c.fog && !c.lit) return refuse(99, "--fog puts a medium into --lit frames: it needs --lit");
    if (c.fog && c.noise) return refuse(99, "--fog cannot be combined with --noise-target: adaptive sampling under a medium is --fog-noise-target T");
    if (grid && ball) return refuse(99, "--fog-grid fills a box: it cannot be combined with --fog-ball");
    if (grid && !box) return refuse(99, "--fog-grid fills the box of --fog-box: it needs --fog SIGMA and --fog-box");
    if (!p.fog_bad.empty()) return refuse(99, p.fog_bad);
    if (grid && !read_grid_file(p.grid_file, cli.fog_grid))
        return refuse(99, "--fog-grid takes a FILE of the header \"VOL1\\nnx ny nz\\n\" (each 1 … " + std::to_string(RT_VOLUME_MAX_N) +
                              ") and then exactly nx*ny*nz little-endian float32 densities, finite and not negative: " + p.grid_file);
    if (c.fog_glow && heat && !read_grid_file(p.heat_file, cli.fog_heat)) return refuse(99, "--fog-heat takes a FILE of --fog-grid's format, finite and not negative: " + p.heat_file);
    if (c.fog_glow && heat && (c.fog_heat.n[0] != c.fog_grid.n[0] || c.fog_heat.n[1] != c.fog_grid.n[1] || c.fog_heat.n[2] != c.fog_grid.n[2]))
        return refuse(99, "--fog-heat: the heat grid's dimensions differ from the density grid's: " + p.heat_file);
    if (c.fog_glow && !(c.fog_sigma > 0.0f) && (c.fog_glow_radiance[0] > 0.0f || c.fog_glow_radiance[1] > 0.0f || c.fog_glow_radiance[2] > 0.0f))
        return refuse(99, "--fog-glow needs --fog SIGMA with SIGMA > 0: a glow without extinction has no kernel");
    // --glossy
    if (c.glossy && !c.lit && !c.nee && !(c.env && !p.env_mode_path))
        return refuse(99, "--glossy takes light samples at METAL's reflect branch: it needs --nee, --env (mode mis or light) or --lit");
    // --env, --env-mode, --env-scale, --env-up
    if (!c.env && !p.env_dash_word.empty()) return refuse(99, p.env_dash_word + " needs --env FILE");          // the last element that begins with --env-
    if (!p.env_bad.empty()) return refuse(99, p.env_bad);
    if (c.env && (env_devices || (!c.lit && (many || adaptive || c.denoise_temporal || p.any({"--nee", "--lens", "--motion-blur"})))))
        return refuse(99, "--env renders frame after frame on one GPU: it cannot be combined with --nee, --lens, --motion-blur, "
                          "--adaptive, --denoise-temporal, --devices, --shard or RTP_DEVICES");
    std::string error;
    if (c.env && !load_hdr_image(c.env_file, cli.env_image, error)) return refuse(99, "--env: " + error);
    if (c.env && !c.lit) return accept(Cli::Driver::lens);          // oddity: accepted here, whatever the checks below would say
    // --nee, --light-tree
    const bool one_gpu_others = env_devices || many || adaptive || c.denoise_temporal;
    if (c.light_tree && !c.nee && !c.lit) return refuse(99, "--light-tree picks the emitter of a light sample: it needs --nee or --lit");
    if (c.nee && p.nee_bad) return refuse(99, "--nee takes mis (default) or light");
    if (c.nee && !c.lit && (one_gpu_others || p.any({"--lens", "--motion-blur"})))
        return refuse(99, "--nee renders frame after frame on one GPU: it cannot be combined with --lens, --motion-blur, "
                          "--adaptive, --denoise-temporal, --devices, --shard or RTP_DEVICES");
    if (c.nee && !c.lit) return accept(Cli::Driver::lens);          // oddity: accepted here, like --env
    // --lens, --motion-blur, and --lit's frames
    if (c.lens || c.motion_blur || c.lit) {
        if (p.lens_bad) return refuse(99, "--lens takes R:F (R >= 0, F > 0, finite) and --motion-blur takes S (0 < S <= 1)");
        if (one_gpu_others)
            return refuse(99, "--lens / --motion-blur render frame after frame on one GPU: they cannot be combined with "
                              "--denoise-temporal, --adaptive, --devices, --shard or RTP_DEVICES");
        return accept(Cli::Driver::lens);
    }
    // the frame-after-frame loop and the drivers beside it: exit code 2
    if (c.denoise && c.denoise_temporal) return refuse(2, "--denoise and --denoise-temporal both write <frame>.denoised: choose one");
    if ((c.aov || c.denoise || c.denoise_temporal) && (many || c.devices > 0))
        return refuse(2, std::string(c.aov ? "--aov" : c.denoise ? "--denoise" : "--denoise-temporal") +
                             " renders frame after frame on one GPU: it cannot be combined with --devices, --shard or RTP_DEVICES");
    if (p.adaptive_valued) {
        if (p.adaptive_spp_bad) return refuse(2, "--adaptive-spp takes min:batch:max");
        if (c.aov || c.denoise || c.denoise_temporal || c.devices > 0)          // oddity: --devices 0, or --devices as the last element, passes
            return refuse(2, "--adaptive renders frame after frame on one GPU: it cannot be combined with --aov, --denoise, "
                             "--denoise-temporal, --devices, --shard or RTP_DEVICES");
        if (p.has("--shard")) return refuse(2, "--adaptive cannot be combined with --shard");
        return accept(Cli::Driver::adaptive);
    }
    if (p.shard_valued) return accept(Cli::Driver::sharded);
    if (c.devices > 0) return accept(Cli::Driver::pipelined);
    return accept(Cli::Driver::frames);
}

}  // namespace rtp
