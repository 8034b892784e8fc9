// main.cpp -- headless render-loop entry point with the shape of the reference's main
// (src/main.cpp:9-31): parse arguments -> Window() -> Scene::parse(-i file) -> Window::mainloop().
// Extra flags drive what the reference hard-codes or leaves to the shader defaults.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "scene.h"
#include "window.h"

using namespace glrt;

static void usage(const char *exe) {
    std::printf("usage: %s -i scene.json [-s N] [--max-depth D] [--spp N] [--frames F] [--frames-in-flight B] [--bvh sah|sah-reinsert|sah-gpu|lbvh|sah-levels-cpu|lbvh-cpu|reference] [--order-by-hits] [--out file.png] [--save-every-frame] [--device G | --gpus N | --devices a,b,..] [--extensions] [--texture-wavefront] [--whitted] [--enable-volume] [--volume-wavefront] [--adaptive THRESHOLD | --adaptive-variance THRESHOLD [--min-spp N]] [--denoise | --denoise-variance [--denoise-iters N]] [--tonemap clamp|reinhard|aces [--exposure X] [--auto-exposure]] [--bloom [--bloom-threshold T] [--bloom-strength S] [--bloom-levels N]] [--reweight [--reweight-kappa K] [--reweight-start S]] [--animate FILE [--carry-history]]\n"
                "  -i, --input             scene description (JSON; schema: SURVEY.md Appendix C)            [required]\n"
                "  -s, --sample-per-cycle  accepted for compatibility; like the reference (main.cpp:13) it is not read\n"
                "      --max-depth D       u_maxDepth (default 16, the reference shader's default)\n"
                "      --spp N             samples per pixel per frame, u_nSamples (default 1 as window.cpp:239)\n"
                "      --frames F          frames to accumulate before exiting (default 16)\n"
                "      --frames-in-flight B frames per launch of the render kernel (default 16; same pixels as 1)\n"
                "      --bvh KIND          sah (CPU, default) | sah-reinsert (sah + insertion-based optimisation: seconds to build, config 5 renders 3 percent faster) | sah-gpu (binned SAH built on the GPU) | lbvh (linear BVH built on the GPU) | sah-levels-cpu | lbvh-cpu | reference (the reference host's own tree, its builder restated: exact ties and grazing-ray box misses as under the reference host; a worse tree, never re-ordered)\n"
                "      --order-by-hits     before the first frame, order every fork's children by the closest hits of one calibration frame (config 5: -1 percent per frame)\n"
                "      --out file.png      tonemapped output (default output.png, written after the last frame)\n"
                "      --save-every-frame  write the image after every frame, one frame per launch (the reference's cadence, window.cpp:164)\n"
                "      --device G          HIP device ordinal (default: current)\n"
                "      --gpus N            render on HIP devices 0..N-1: interleaved 8-row stripes, gathered when the image is written\n"
                "      --devices a,b,..    the same with an explicit device list (an ordinal may repeat)\n"
                "      --extensions        accept what the reference does not have: shapes of type \"sphere\" (center, radius) and the material\n"
                "                          \"dielectric\" (ior, tint), and a diffuse shape's \"texture\": {\"file\": x.ppm | x.pfm, \"filter\", \"wrap\", \"srgb\"}\n"
                "                          (looked up at the OBJ's vt coordinates); parity with the reference is not defined for such scenes;\n"
                "                          a diffuse or conductor shape's \"cutout\": {\"file\": mask.ppm | mask.pfm, \"channel\": \"r\" | \"g\" | \"b\", \"cutoff\",\n"
                "                          \"filter\", \"wrap\"} (an alpha test inside the ray search: hits count where the mask's channel >= cutoff);\n"
                "                          an emitter shape's \"emission_map\": {\"file\": x.ppm | x.pfm, \"filter\", \"wrap\", \"srgb\"} (multiplies the emission,\n"
                "                          where the emitter is seen and where it is sampled as a light)\n"
                "                          and the top-level \"environment\": {\"file\": x.pfm | x.ppm, \"layout\": \"latlong\" | \"octahedral\", \"size\", \"mode\", \"scale\",\n"
                "                          \"rotate_y\", \"light_pick\", \"filter\", \"srgb\"} (light from an HDR map where a ray leaves the scene; not with --enable-volume)\n"
                "      --env-mode M        with --extensions: \"escape\" or \"sampled\", overrides the \"environment\" block's \"mode\"\n"
                "      --whitted           with --extensions: Whitted-style transport (direct light at diffuse surfaces, specular bounces only)\n"
                "      --enable-volume     render the participating media of \"media\" shapes: the reference's ENABLE_VOLUME switch (raytrace.frag:4);\n"
                "                          their VOL files are read (a missing one is an error only with this flag)\n"
                "      --volume-wavefront  with --enable-volume: render the media on the wavefront kernel (frames in flight, fed launches; the same image as\n"
                "                          the persistent megakernel, the default).  --enable-volume --adaptive T turns it on by itself\n"
                "      --texture-wavefront  with --extensions: render textured shapes (material maps included) on the wavefront kernel (frames in flight, fed\n"
                "                          launches; the same image as the textured megakernel, the default); scenes with spheres, dielectrics or an environment\n"
                "                          render as without it\n"
                "      --adaptive T        adaptive sampling: bursts of --frames-in-flight frames on the 8x8 tiles whose error is above T only, until no tile is\n"
                "                          active or --frames frames have been issued; an \"Adaptive:\" line per burst (not with --save-every-frame)\n"
                "      --adaptive-variance T  the same bursts with the tiles selected by the variance of their pixels' mean luminance (the moments plane that\n"
                "                          --denoise-variance filters by): a tile retires once its mean standard error over the root of its luminance is at most T --\n"
                "                          not --adaptive's T.  One device; not with --adaptive or --save-every-frame; composes with --denoise-variance, --bloom, --tonemap\n"
                "      --min-spp N         with --adaptive or --adaptive-variance: samples every pixel of a tile needs before the tile may retire (default 2, at least 2)\n"
                "      --denoise           write the denoised image: feature planes once before the first frame, then the edge-avoiding a-trous filter over the\n"
                "                          accumulated mean (one device; not with --save-every-frame).  Without it the output is what it always was\n"
                "      --denoise-variance  write the variance-guided image instead: the frames are rendered with glrtx_render_moments in bursts of --frames-in-flight\n"
                "                          (at most 1024) frames, then SVGF's filter runs over the mean (one device; not with --denoise, --adaptive,\n"
                "                          --save-every-frame, extension or volume scenes)\n"
                "      --denoise-iters N   with --denoise or --denoise-variance: filter iterations, 1..6 (default 5)\n"
                "      --tonemap OP        write the image through a tone curve: clamp (the plain resolve's), reinhard (extended, white point 4) or aces (Narkowicz's fit);\n"
                "                          the denoised image with --denoise / --denoise-variance (one device; not with --save-every-frame).  Without it the output is\n"
                "                          what it always was\n"
                "      --exposure X        with --tonemap: linear multiplier in front of the curve (default 1)\n"
                "      --auto-exposure     with --tonemap: multiply by the exposure measured from the image's luminance histogram as well (key 0.18)\n"
                "      --bloom             add a glow around over-bright pixels to the linear image in front of the curve (an image pyramid: glrtx_bloom); after\n"
                "                          --denoise* if given; without --tonemap the curve is clamp (one device; not with --save-every-frame)\n"
                "      --bloom-threshold T with --bloom: luminance above which a pixel glows, >= 0 (default 1)\n"
                "      --bloom-strength S  with --bloom: weight of the glow, 0..1e4 (default 0.25)\n"
                "      --bloom-levels N    with --bloom: pyramid levels, 1..8 (default 5)\n"
                "      --reweight          write the firefly re-weighted image: the frames are rendered with glrtx_render_cascades in bursts of --frames-in-flight (at\n"
                "                          most 1024) frames, every sample binned by luminance, and a brightness level counts only as far as the 3x3 neighbourhood\n"
                "                          expects it; goes through --bloom / --tonemap as a denoised image does (one device; not with --denoise, --denoise-variance,\n"
                "                          --adaptive, --adaptive-variance, --enable-volume or --save-every-frame)\n"
                "      --reweight-kappa K  with --reweight: samples the neighbourhood must hold besides one for a level to count in full, > 0 (default 4)\n"
                "      --reweight-start S  with --reweight: luminance bound of the first cascade, 2^-20 .. 2^20 (default 1); the others are S * 8^k\n"
                "      --animate FILE      pose the scene's shapes on the device step by step (glrtx_pose): FILE is JSON, {\"steps\": [{\"matrices\": [[shape, m0, ..., m11], ...],\n"
                "                          \"camera\": {...}}, ...]} -- shape: index into the scene file's \"scene\" array, m: row-major 3x4, unlisted shapes keep the identity,\n"
                "                          \"camera\" optional with the scene file's keys.  Every step renders --frames frames and writes <out stem>_<step, 4 digits>.<ext> as a\n"
                "                          still run would under the same --denoise* / --bloom / --tonemap (one device; not with --adaptive*, --reweight, --enable-volume,\n"
                "                          --extensions or --save-every-frame).  Morph targets: a top-level \"targets\": [{\"shape\": i, \"file\": \"x.obj\"}, ...] and per step\n"
                "                          \"weights\": [[target, w], ...] blend the shapes' vertices towards the targets' before the pose (glrtx_pose_morph), at most 64\n"
                "                          targets; with a top-level \"sparse_targets\": true at most 1024, each kept as the list of the vertices it moves\n"
                "                          (glrtx_upload_morph_targets_sparse); a top-level \"rebuild_normals\": true rebuilds every step's shading normals\n"
                "                          from its moved faces (glrtx_set_pose_normals), welded by position and normal or, with \"weld\": \"positions\", by\n"
                "                          position alone\n"
                "      --carry-history     with --animate: keep the accumulator across the steps by motion-aware reprojection (glrtx_reproject_motion) instead of clearing\n"
                "                          it; moments are tracked, so --denoise-variance composes (not with --denoise)\n", exe);
}

int main(int argc, char **argv) {
    std::string input, out = "output.png";
    int depth = 16, spp = 1, frames = 16, device = -1, in_flight = 0;
    int env_mode = -1;  // --env-mode: GLRTX_ENV_*, -1 the scene file's
    bool every_frame = false, extensions = false, whitted = false, order_by_hits = false, volume = false, adaptive = false, adaptive_variance = false, min_spp_given = false, volume_wavefront = false, texture_wavefront = false;
    float adapt_threshold = 0.0f;
    int min_spp = 2;
    bool denoise = false, denoise_variance = false;
    int denoise_iters = 0;
    int tonemap_op = -1;
    float exposure = 1.0f;
    bool exposure_given = false, auto_exposure = false;
    bool bloom = false, bloom_opt = false;
    bool reweight = false, reweight_opt = false;
    float reweight_kappa = 4.0f, reweight_start = 1.0f;
    float bloom_threshold = 1.0f, bloom_strength = 0.25f;
    int bloom_levels = 5;
    std::vector<int> devices;
    std::string bvh, animate;
    bool carry_history = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&](const char *name) -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", name); std::exit(1); }
            return argv[++i];
        };
        if (a == "-i" || a == "--input") input = next("--input");
        else if (a == "-s" || a == "--sample-per-cycle") (void)next("--sample-per-cycle");
        else if (a == "--max-depth") depth = std::atoi(next("--max-depth"));
        else if (a == "--spp") spp = std::atoi(next("--spp"));
        else if (a == "--frames") frames = std::atoi(next("--frames"));
        else if (a == "--frames-in-flight") in_flight = std::atoi(next("--frames-in-flight"));
        else if (a == "--out") out = next("--out");
        else if (a == "--bvh") bvh = next("--bvh");
        else if (a == "--device") device = std::atoi(next("--device"));
        else if (a == "--save-every-frame") every_frame = true;
        else if (a == "--order-by-hits") order_by_hits = true;
        else if (a == "--extensions") extensions = true;
        else if (a == "--whitted") { extensions = true; whitted = true; }
        else if (a == "--env-mode") {
            const std::string m = next("--env-mode");
            if (m != "escape" && m != "sampled") { std::fprintf(stderr, "--env-mode is \"escape\" or \"sampled\"\n"); return 1; }
            env_mode = m == "sampled" ? 1 : 0;
        }
        else if (a == "--enable-volume") volume = true;
        else if (a == "--volume-wavefront") volume_wavefront = true;
        else if (a == "--texture-wavefront") texture_wavefront = true;
        else if (a == "--adaptive") { adaptive = true; adapt_threshold = (float)std::atof(next("--adaptive")); }
        else if (a == "--adaptive-variance") { adaptive_variance = true; adapt_threshold = (float)std::atof(next("--adaptive-variance")); }
        else if (a == "--min-spp") { min_spp = std::atoi(next("--min-spp")); min_spp_given = true; }
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-variance") denoise_variance = true;
        else if (a == "--denoise-iters") denoise_iters = std::atoi(next("--denoise-iters"));
        else if (a == "--tonemap") {
            const std::string op = next("--tonemap");
            tonemap_op = op == "clamp" ? 0 : (op == "reinhard" ? 1 : (op == "aces" ? 2 : -2));
            if (tonemap_op < 0) { std::fprintf(stderr, "--tonemap: clamp, reinhard or aces\n"); return 1; }
        }
        else if (a == "--exposure") { exposure = (float)std::atof(next("--exposure")); exposure_given = true; }
        else if (a == "--auto-exposure") auto_exposure = true;
        else if (a == "--bloom") bloom = true;
        else if (a == "--reweight") reweight = true;
        else if (a == "--animate") animate = next("--animate");
        else if (a == "--carry-history") carry_history = true;
        else if (a == "--reweight-kappa") { reweight_kappa = (float)std::atof(next("--reweight-kappa")); reweight_opt = true; }
        else if (a == "--reweight-start") { reweight_start = (float)std::atof(next("--reweight-start")); reweight_opt = true; }
        else if (a == "--bloom-threshold") { bloom_threshold = (float)std::atof(next("--bloom-threshold")); bloom_opt = true; }
        else if (a == "--bloom-strength") { bloom_strength = (float)std::atof(next("--bloom-strength")); bloom_opt = true; }
        else if (a == "--bloom-levels") { bloom_levels = std::atoi(next("--bloom-levels")); bloom_opt = true; }
        else if (a == "--gpus") { const int n = std::atoi(next("--gpus")); devices.clear(); for (int k = 0; k < n; k++) devices.push_back(k); }
        else if (a == "--devices") {
            devices.clear();
            for (const char *p = next("--devices"); *p;) { devices.push_back(std::atoi(p)); while (*p && *p != ',') p++; if (*p == ',') p++; }
        }
        else { usage(argv[0]); return 1; }
    }
    if (input.empty()) { usage(argv[0]); return 1; }
    if (min_spp_given && !adaptive && !adaptive_variance) { std::fprintf(stderr, "--min-spp needs --adaptive or --adaptive-variance\n"); return 1; }
    if (adaptive_variance && (adaptive || every_frame || devices.size() > 1 || min_spp < 2)) {
        std::fprintf(stderr, "--adaptive-variance: one device, not with --adaptive or --save-every-frame, and --min-spp must be at least 2\n");
        return 1;
    }
    if (adaptive && (every_frame || min_spp < 2)) { std::fprintf(stderr, "--adaptive: not with --save-every-frame, and --min-spp must be at least 2\n"); return 1; }

    if (denoise_iters != 0 && ((!denoise && !denoise_variance) || denoise_iters < 1 || denoise_iters > 6)) {
        std::fprintf(stderr, "--denoise-iters needs --denoise or --denoise-variance and a value in 1..6\n");
        return 1;
    }
    if (denoise && (every_frame || devices.size() > 1)) { std::fprintf(stderr, "--denoise: one device, and not with --save-every-frame\n"); return 1; }
    if (denoise_variance && (denoise || adaptive || every_frame || devices.size() > 1)) {
        std::fprintf(stderr, "--denoise-variance: one device, and not with --denoise, --adaptive or --save-every-frame\n");
        return 1;
    }
    if (denoise_variance && in_flight > 1024) {  // (a burst is one glrtx_render_moments call: as many frames as one launch's seed table takes)
        std::fprintf(stderr, "--denoise-variance: --frames-in-flight %d is above the 1024 frames one glrtx_render_moments burst takes\n", in_flight);
        return 1;
    }
    if (reweight_opt && !reweight) { std::fprintf(stderr, "--reweight-kappa and --reweight-start need --reweight\n"); return 1; }
    if (reweight && (denoise || denoise_variance || adaptive || adaptive_variance || volume || every_frame || devices.size() > 1)) {
        std::fprintf(stderr, "--reweight: one device, and not with --denoise, --denoise-variance, --adaptive, --adaptive-variance, --enable-volume or --save-every-frame\n");
        return 1;
    }
    if (reweight && (!(reweight_kappa > 0.0f) || std::isinf(reweight_kappa) || !(reweight_start >= 0x1p-20f && reweight_start <= 0x1p20f))) {
        std::fprintf(stderr, "--reweight: --reweight-kappa must be a positive finite number and --reweight-start within 2^-20 .. 2^20\n");
        return 1;
    }
    if (reweight && in_flight > 1024) {  // (a burst is one glrtx_render_cascades call, as --denoise-variance's is one glrtx_render_moments call)
        std::fprintf(stderr, "--reweight: --frames-in-flight %d is above the 1024 frames one glrtx_render_cascades burst takes\n", in_flight);
        return 1;
    }
    if (carry_history && animate.empty()) { std::fprintf(stderr, "--carry-history needs --animate\n"); return 1; }
    if (!animate.empty() && (devices.size() > 1 || adaptive || adaptive_variance || reweight || volume || extensions || every_frame)) {
        std::fprintf(stderr, "--animate: one device, and not with --adaptive, --adaptive-variance, --reweight, --enable-volume, --extensions or --save-every-frame\n");
        return 1;
    }
    if (carry_history && denoise) { std::fprintf(stderr, "--carry-history: not with --denoise (the fixed-sigma filter has no moments; use --denoise-variance)\n"); return 1; }
    if (!animate.empty() && (denoise_variance || carry_history) && in_flight > 1024) {
        std::fprintf(stderr, "--animate: --frames-in-flight %d is above the 1024 frames one glrtx_render_moments burst takes\n", in_flight);
        return 1;
    }
    if (bloom_opt && !bloom) { std::fprintf(stderr, "--bloom-threshold, --bloom-strength and --bloom-levels need --bloom\n"); return 1; }
    if (bloom && (every_frame || devices.size() > 1 || !(bloom_threshold >= 0.0f) || std::isinf(bloom_threshold) || !(bloom_strength >= 0.0f && bloom_strength <= 1.0e4f) ||
                  bloom_levels < 1 || bloom_levels > 8)) {
        std::fprintf(stderr, "--bloom: one device, not with --save-every-frame; --bloom-threshold finite and >= 0, --bloom-strength in 0..1e4, --bloom-levels in 1..8\n");
        return 1;
    }
    if ((exposure_given || auto_exposure) && tonemap_op < 0) { std::fprintf(stderr, "--exposure and --auto-exposure need --tonemap\n"); return 1; }
    if (tonemap_op >= 0 && (every_frame || devices.size() > 1 || !(exposure > 0.0f) || std::isinf(exposure))) {
        std::fprintf(stderr, "--tonemap: one device, not with --save-every-frame, and --exposure must be a positive finite number\n");
        return 1;
    }

    auto window = std::make_unique<Window>();
    if (devices.empty()) window->setDevice(device);
    else window->setDevices(devices);
    window->setMaxDepth(depth);
    window->setSamplesPerFrame(spp);
    window->setFrameLimit(frames);
    if (in_flight > 0) window->setFramesInFlight(in_flight);
    window->setOutput(out, every_frame);
    window->setOrderChildrenByHits(order_by_hits);
    if (adaptive) window->setAdaptive(adapt_threshold, min_spp);
    if (adaptive_variance) window->setAdaptiveVariance(adapt_threshold, min_spp);
    window->setVolumeWavefront(volume_wavefront);
    window->setTextureWavefront(texture_wavefront);
    if (denoise) window->setDenoise(denoise_iters);
    if (denoise_variance) window->setDenoiseVariance(denoise_iters);
    if (tonemap_op >= 0) window->setTonemap(tonemap_op, exposure, auto_exposure);
    if (bloom) window->setBloom(bloom_threshold, bloom_strength, bloom_levels);
    if (reweight) window->setReweight(reweight_kappa, reweight_start);
    if (!animate.empty()) window->setAnimation(animate, carry_history);

    auto scene = std::make_shared<Scene>();
    if (!bvh.empty()) scene->setBvhBuilder(bvh);
    scene->enableExtensions(extensions);
    scene->setWhitted(whitted);
    scene->setEnvMode(env_mode);
    scene->enableVolume(volume);
    scene->parse(input);

    window->mainloop(scene);
    std::printf("[INFO] %d frames, %.3f ms per frame (wall time between the last two waits for the device, averaged over the frames issued in between), %llu rays\n", frames, window->lastFrameMs(), window->raysTraced());
    return 0;
}
