// main.cpp — CLI with the reference's modes (src/main.cu:572-606): no argument or --gpu reads a
// scene description from stdin and renders every frame on the GPU; --default prints the default
// description.  --cpu is the reference's single-threaded CPU loop: this build ships no CPU
// render path (its CPU restatement lives under oracle/ as a test checker only), so --cpu fails
// loudly instead of silently rendering on the host.
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "camera.h"
#include "cli.h"
#include "scene_builder.h"
#include "scene_params.h"


namespace {

void set_adaptive(rt_adaptive_params &ap, float threshold, const rtp::CliSpp &spp) {
    rt_adaptive_params_init(&ap);
    ap.threshold = threshold;
    if (!spp.given) return;
    ap.min_spp = spp.min_spp;
    ap.batch_spp = spp.batch_spp;
    ap.max_spp = spp.max_spp;
}

int creation_failed(const std::string &what) {
    std::cerr << "rtp_main: " << what << ": " << rt_get_last_error_string() << "\n";
    return 99;
}

// Driver lens: the rt_*_params of an accepted command line, its device objects (made only now, after the last refusal, in this order:
// environment, density grid, heat grid, glow sampler) and the frames.  --lit takes every member; without it one of --env, --nee or the
// bare lens.
int render_lens(const rtp::SceneParams &params, const rt_scene_desc &desc, const rtp::Cli &cli) {
    rtp::FrameJob job;
    rt_lens_params lens;
    rt_lens_params_init(&lens);
    if (cli.lens) {
        lens.lens_radius = cli.lens_radius;
        lens.focus_distance = cli.lens_focus;
    }
    job.lens = &lens;
    job.shutter = cli.shutter;
    job.aov = cli.aov;
    job.denoise = cli.denoise;
    rt_nee_params nee;
    rt_nee_params_init(&nee);
    if (cli.nee_mis >= 0) nee.mis = cli.nee_mis;
    nee.select = cli.light_tree ? 1 : 0;
    nee.glossy = cli.glossy ? 1 : 0;
    rt_env_params ep;
    rt_env_params_init(&ep);
    rt_env *env = nullptr;
    if (cli.env) {
        if (cli.env_mode >= 0) ep.mode = cli.env_mode;
        if (cli.env_scale_given) ep.scale = cli.env_scale;
        if (cli.env_up_z) {
            const float z_up[9] = {1, 0, 0, 0, 0, 1, 0, -1, 0};        // environment y = world z
            for (int k = 0; k < 9; ++k) ep.rot[k] = z_up[k];
        }
        if (cli.glossy && ep.mode != 0) ep.glossy = 1;
        std::vector<float> map(static_cast<size_t>(cli.env_n) * cli.env_n * 3);
        if (rt_env_from_equirect(cli.env_image.rgb.data(), cli.env_image.width, cli.env_image.height, cli.env_n, map.data()) != RT_OK ||
            rt_env_create(map.data(), cli.env_n, &env) != RT_OK)
            return creation_failed("--env: " + cli.env_file);
    }
    rt_volume *volume = nullptr, *heat = nullptr;
    rt_glow_sampler *sampler = nullptr;
    const rtp::CliGrid &g = cli.fog_grid, &h = cli.fog_heat;
    if (!g.cells.empty() && rt_volume_create(g.cells.data(), g.n[0], g.n[1], g.n[2], &volume) != RT_OK) return creation_failed("--fog-grid");
    if (!h.cells.empty() && rt_volume_create(h.cells.data(), h.n[0], h.n[1], h.n[2], &heat) != RT_OK) return creation_failed("--fog-heat");
    if (cli.fog_glow_sample && rt_glow_sampler_create(volume, cli.fog_glow_source, heat, &sampler) != RT_OK) return creation_failed("--fog-glow-sample");

    rt_lit_params lit;
    rt_lit_params_init(&lit);
    lit.nee = &nee;
    lit.env = env;
    lit.env_params = &ep;
    rt_adaptive_params noise;
    if (cli.fog_noise) set_adaptive(noise, cli.fog_noise_threshold, cli.fog_noise_spp);
    else set_adaptive(noise, cli.noise_threshold, cli.noise_spp);
    rt_adaptive_params fog_adaptive;
    set_adaptive(fog_adaptive, cli.fog_adaptive_threshold, cli.fog_adaptive_spp);
    rt_stop_params stop;
    rt_stop_params_init(&stop);
    stop.rule = cli.stop_rule;
    rt_medium_params fog;
    rt_medium_params_init(&fog);
    fog.region = cli.fog_region;
    fog.sigma_t = cli.fog_sigma;
    fog.albedo[0] = fog.albedo[1] = fog.albedo[2] = cli.fog_albedo;
    fog.g = cli.fog_g;
    rt_chroma_params tint;
    rt_chroma_params_init(&tint);
    rt_glow_params glow;
    rt_glow_params_init(&glow);
    glow.source = cli.fog_glow_source;
    for (int k = 0; k < 3; ++k) {
        fog.a[k] = cli.fog_a[k];
        fog.b[k] = cli.fog_b[k];
        tint.tint[k] = cli.fog_tint_rgb[k];
        glow.radiance[k] = cli.fog_glow_radiance[k];
    }
    rt_glow_sample_params glow_sample;
    rt_glow_sample_params_init(&glow_sample);
    glow_sample.sample = 1;
    glow_sample.mis = cli.fog_glow_sample_mis;
    if (cli.lit) {
        job.lit = &lit;
        job.noise = cli.fog_noise || cli.noise ? &noise : nullptr;
        job.denoise_adaptive = cli.denoise_adaptive;
        job.stop = &stop;
        job.denoise_adaptive_temporal = cli.denoise_adaptive_temporal;
        job.medium = cli.fog ? &fog : nullptr;
        job.stop_history = cli.stop_history;
        job.volume = volume;
        job.fog_denoise = cli.fog_denoise;
        job.chroma = cli.fog_tint ? &tint : nullptr;
        job.glow = cli.fog_glow ? &glow : nullptr;
        job.heat = heat;
        job.glow_sample = cli.fog_glow_sample ? &glow_sample : nullptr;
        job.sampler = sampler;
        job.fog_adaptive = cli.fog_adaptive ? &fog_adaptive : nullptr;
        job.split = cli.split;
    } else if (cli.env) {
        job.env = env;
        job.env_params = &ep;
    } else if (cli.nee) {
        job.nee = &nee;
    }
    rtp::gpu_render_lens(params, desc, job);
    rt_glow_sampler_destroy(sampler);
    rt_volume_destroy(heat);
    rt_volume_destroy(volume);
    rt_env_destroy(env);
    return 0;
}

}  // namespace

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

    rtp::SceneParams params = rtp::read_scene_params(std::cin);          // (before the command line is judged: a malformed scene fails first)
    rtp::HostScene host;
    rtp::build_config_scene(params, "", host);
    const rt_scene_desc desc = host.desc();

    rtp::Cli cli;
    rtp::CliRefusal refusal;
    if (!rtp::parse_cli(argc, argv, getenv("RTP_DEVICES"), cli, refusal)) {
        std::cerr << "rtp_main: " << refusal.text << "\n";
        return refusal.code;
    }
    switch (cli.driver) {
    case rtp::Cli::Driver::lens:
        return render_lens(params, desc, cli);
    case rtp::Cli::Driver::adaptive: {
        rtp::FrameJob job;
        rt_adaptive_params ap;
        set_adaptive(ap, cli.adaptive_threshold, cli.adaptive_spp);
        rt_stop_params stop;
        rt_stop_params_init(&stop);
        stop.rule = cli.stop_rule;
        job.noise = &ap;
        job.stop = &stop;
        job.denoise_adaptive = cli.denoise_adaptive;
        job.denoise_adaptive_temporal = cli.denoise_adaptive_temporal;
        job.stop_history = cli.stop_history;
        rtp::gpu_render_adaptive(params, desc, job);
        return 0;
    }
    case rtp::Cli::Driver::sharded:
        rtp::gpu_render_sharded(params, desc, cli.shards);
        return 0;
    case rtp::Cli::Driver::pipelined:
        rtp::gpu_render_pipelined(params, desc, cli.devices);
        return 0;
    case rtp::Cli::Driver::frames:
        break;
    }
    rt_scene *scene = nullptr;
    RTP_CHECK(rt_scene_create(&desc, &scene));
    rtp::bind_scene(scene);
    rtp::gpu_render(params, cli.aov, cli.denoise, cli.denoise_temporal);
    RTP_CHECK(rt_scene_destroy(scene));
    return 0;
}
