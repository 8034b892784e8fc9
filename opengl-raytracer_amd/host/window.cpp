// window.cpp -- headless glrt::Window over the C-ABI HIP layer.  Structure follows the reference's
// Window (src/core/window.cpp): mainloop :105-182, render :213-318, resetBuffer :366-381,
// saveCurrentFrame :383-414; every GL call is replaced by its glrtx_* counterpart.
#include "window.h"

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "glrt_host.h"
#include "glrtx.h"

namespace glrt {

#define GLRTX_CHECK(call)                                                                        \
    do {                                                                                         \
        if ((call) != GLRTX_OK) GLRT_FatalError("%s: %s", #call, glrtx_group_last_error(grp_));  \
    } while (0)

Window::Window() {
    if (const char *e = std::getenv("GLRT_FRAMES")) frameLimit_ = std::atoi(e);
    if (const char *e = std::getenv("GLRT_MAX_DEPTH")) maxDepth_ = std::atoi(e);
    if (const char *e = std::getenv("GLRT_FRAMES_IN_FLIGHT")) setFramesInFlight(std::atoi(e));
    if (const char *e = std::getenv("GLRT_GPUS")) {
        const int n = std::atoi(e);
        if (n > 1) { devices_.clear(); for (int i = 0; i < n; i++) devices_.push_back(i); }
    }
}

Window::~Window() {
    if (grp_) glrtx_group_destroy(grp_);
}

unsigned long long Window::raysTraced() const {
    glrtx_stats st;
    if (!grp_ || glrtx_group_get_stats(grp_, &st) != GLRTX_OK) return 0;
    return st.rays;
}

// The scene's textures (Scene::TextureSpec; extensions only) as one set on every member, after the scene: launches then run on the extension megakernel
void Window::uploadTextures() {
    if (scene->textures_.empty() && scene->maps_.empty() && scene->cutouts_.empty() && scene->emissionMaps_.empty()) return;
    std::vector<glrtx_texture> desc;
    std::vector<unsigned char> blob;
    std::vector<int32_t> bind(scene->materials.size(), -1);
    for (const Scene::TextureSpec &t : scene->textures_) {
        blob.resize((blob.size() + 15) / 16 * 16, 0);
        desc.push_back(glrtx_texture{(uint64_t)blob.size(), t.image.width, t.image.height, t.format, t.wrap, t.wrap, t.filter});
        blob.insert(blob.end(), t.image.texels.begin(), t.image.texels.end());
        bind[t.material] = (int32_t)desc.size() - 1;
    }
    // the material maps' images behind them in the same set (Scene::MapSpec), bound with a second call: the set may bind no albedo at all
    std::vector<glrtx_material_map> maps(scene->materials.size(), glrtx_material_map{-1, -1, 1.0f, 0});
    for (const Scene::MapSpec &t : scene->maps_) {
        blob.resize((blob.size() + 15) / 16 * 16, 0);
        desc.push_back(glrtx_texture{(uint64_t)blob.size(), t.image.width, t.image.height, t.format, t.wrap, t.wrap, t.filter});
        blob.insert(blob.end(), t.image.texels.begin(), t.image.texels.end());
        if (t.roughness) maps[t.material].roughness = (int32_t)desc.size() - 1;
        else { maps[t.material].normal = (int32_t)desc.size() - 1; maps[t.material].normal_scale = t.scale; }
    }
    // ... and the cutout masks behind those (Scene::CutoutSpec), bound with a third call
    std::vector<glrtx_cutout> cuts(scene->materials.size(), glrtx_cutout{-1, 0, 0.5f, 0});
    for (const Scene::CutoutSpec &t : scene->cutouts_) {
        blob.resize((blob.size() + 15) / 16 * 16, 0);
        desc.push_back(glrtx_texture{(uint64_t)blob.size(), t.image.width, t.image.height, t.format, t.wrap, t.wrap, t.filter});
        blob.insert(blob.end(), t.image.texels.begin(), t.image.texels.end());
        cuts[t.material] = glrtx_cutout{(int32_t)desc.size() - 1, t.channel, t.cutoff, 0};
    }
    // ... and the emitters' emission maps behind those (Scene::emissionMapSpecs), bound with a fourth call
    std::vector<int32_t> emit(scene->materials.size(), -1);
    for (const Scene::TextureSpec &t : scene->emissionMaps_) {
        blob.resize((blob.size() + 15) / 16 * 16, 0);
        desc.push_back(glrtx_texture{(uint64_t)blob.size(), t.image.width, t.image.height, t.format, t.wrap, t.wrap, t.filter});
        blob.insert(blob.end(), t.image.texels.begin(), t.image.texels.end());
        emit[t.material] = (int32_t)desc.size() - 1;
    }
    for (int i = 0; i < glrtx_group_size(grp_); i++) {
        glrtx_ctx *c = glrtx_group_ctx(grp_, i);
        if (glrtx_upload_textures(c, desc.data(), desc.size(), blob.data(), blob.size(), bind.data(), bind.size()) != GLRTX_OK)
            GLRT_FatalError("glrtx_upload_textures: %s", glrtx_last_error(c));
        if (!scene->maps_.empty() && glrtx_bind_material_maps(c, maps.data(), maps.size()) != GLRTX_OK)
            GLRT_FatalError("glrtx_bind_material_maps: %s", glrtx_last_error(c));
        if (!scene->cutouts_.empty() && glrtx_bind_cutouts(c, cuts.data(), cuts.size()) != GLRTX_OK)
            GLRT_FatalError("glrtx_bind_cutouts: %s", glrtx_last_error(c));
        if (!scene->emissionMaps_.empty() && glrtx_bind_emission_maps(c, emit.data(), emit.size()) != GLRTX_OK)
            GLRT_FatalError("glrtx_bind_emission_maps: %s", glrtx_last_error(c));
    }
    if (!scene->emissionMaps_.empty()) GLRT_Info("emission maps: %zu (not part of the reference)", scene->emissionMaps_.size());
    if (!scene->cutouts_.empty()) GLRT_Info("cutouts: %zu (not part of the reference)", scene->cutouts_.size());
    if (!scene->maps_.empty()) GLRT_Info("material maps: %zu (not part of the reference)", scene->maps_.size());
    GLRT_Info("textures: %zu, %zu texel bytes (not part of the reference)", desc.size(), blob.size());
}

// The scene's environment (Scene::EnvironmentSpec; extensions only) on every member, after the scene: launches then run on the extension megakernel
void Window::uploadEnvironment() {
    const Scene::EnvironmentSpec &e = scene->environment_;
    if (!e.present) return;
    const glrtx_texture map{0, e.size, e.size, e.format, GLRTX_TEX_CLAMP, GLRTX_TEX_CLAMP, e.filter};
    glrtx_env_cfg cfg{};
    cfg.mode = e.mode;
    cfg.grid = 0;
    cfg.light_pick = e.lightPick;
    std::memcpy(cfg.scale, e.scale, sizeof cfg.scale);
    // a turn about +y; quarter turns exactly (the same words as glrt_amd.host.env_cfg(rotate_y=..))
    const double a = (double)e.rotateY * 3.14159265358979323846 / 180.0;
    float cs = (float)std::cos(a), sn = (float)std::sin(a);
    if (std::fmod((double)e.rotateY, 90.0) == 0.0) { cs = (float)std::round(std::cos(a)); sn = (float)std::round(std::sin(a)); }
    const float R[9] = {cs, 0.0f, 0.0f - sn, 0.0f, 1.0f, 0.0f, sn, 0.0f, cs};
    std::memcpy(cfg.rotation, R, sizeof R);
    for (int i = 0; i < glrtx_group_size(grp_); i++) {
        glrtx_ctx *c = glrtx_group_ctx(grp_, i);
        if (glrtx_upload_environment(c, &map, e.texels.data(), e.texels.size(), &cfg) != GLRTX_OK)
            GLRT_FatalError("glrtx_upload_environment: %s", glrtx_last_error(c));
    }
    GLRT_Info("environment: %d x %d texels, %s mode (not part of the reference)", e.size, e.size, e.mode == GLRTX_ENV_SAMPLED ? "sampled" : "escape");
}

void Window::mainloop(const std::shared_ptr<Scene> &scene_, double fps) {
    (void)fps;  // the reference's default fps = -1 renders every iteration (window.cpp:126); so do we
    scene = scene_;
    if (!grp_ && glrtx_group_create(&grp_, devices_.data(), (int)devices_.size()) != GLRTX_OK)
        GLRT_FatalError("glrtx_group_create: %s", glrtx_group_last_error(nullptr));
    // scene upload: the five buffers Scene::parse handed to TextureBuffer::setData (scene.cpp:254-269)
    GLRTX_CHECK(glrtx_group_upload_scene(
        grp_, scene->vertices.empty() ? nullptr : &scene->vertices[0].pos[0], scene->vertices.size(),
        scene->triangles.empty() ? nullptr : &scene->triangles[0].indices[0], scene->triangles.size(),
        scene->materials.empty() ? nullptr : &scene->materials[0].type[0], scene->materials.size(),
        scene->lights.empty() ? nullptr : &scene->lights[0].indices[0], scene->lights.size(),
        scene->nodes.empty() ? nullptr : &scene->nodes[0].bboxMin[0], scene->nodes.size()));
    // the volume of the media materials (Scene::enableVolume): the reference's bindings of volumes[0] (window.cpp:271-286) -- the first nx*ny*nz floats of each
    // file (glTexSubImage3D with GL_RED), u_densityMax = the density file's maximum, the JSON's bbox
    if (scene->hasVolume_) {
        const VolumeGrid &d = scene->volDensity_, &t = scene->volTemperature_;
        const Scene::VolumeSpec &v = scene->volumeSpecs_[0];
        GLRTX_CHECK(glrtx_group_upload_volume(grp_, d.texels(), t.texels(), d.nx, d.ny, d.nz, v.bboxMin, v.bboxMax, d.maxValue()));
        GLRT_Info("volume: %d x %d x %d voxels, density max %g", d.nx, d.ny, d.nz, d.maxValue());
    }
    // extensions the scene asked for (Scene::enableExtensions; none in a reference scene): analytic spheres, dielectric, Whitted; the volume flag
    if (!scene->spheres.empty() || scene->hasDielectric_ || scene->whitted_ || scene->hasVolume_) {
        const int flags = (scene->hasDielectric_ ? GLRTX_EXT_DIELECTRIC : 0) | (scene->whitted_ ? GLRTX_EXT_WHITTED : 0) | (scene->hasVolume_ ? GLRTX_EXT_VOLUME : 0);
        for (int i = 0; i < glrtx_group_size(grp_); i++) {
            glrtx_ctx *c = glrtx_group_ctx(grp_, i);
            if (glrtx_upload_spheres(c, scene->spheres.empty() ? nullptr : scene->spheres.data(), scene->spheres.size() / 5) != GLRTX_OK ||
                glrtx_set_extensions(c, flags) != GLRTX_OK)
                GLRT_FatalError("extensions: %s", glrtx_last_error(c));
            // the volume on the wavefront kernel: asked for, or needed -- adaptive sampling has a tile list only there
            if ((volumeWavefront_ || (adaptive_ && scene->hasVolume_)) && glrtx_set_volume_wavefront(c, 1) != GLRTX_OK)
                GLRT_FatalError("glrtx_set_volume_wavefront: %s", glrtx_last_error(c));
        }
        if (!scene->spheres.empty() || scene->hasDielectric_ || scene->whitted_)
            GLRT_Info("extensions: %zu analytic spheres%s%s (not part of the reference)", scene->spheres.size() / 5,
                      scene->hasDielectric_ ? ", dielectric" : "", scene->whitted_ ? ", Whitted termination" : "");
    }
    uploadTextures();
    if (textureWavefront_) {  // the set on the wavefront kernel, on every member (a switch: it takes effect on the launches that can route there)
        for (int i = 0; i < glrtx_group_size(grp_); i++)
            if (glrtx_set_texture_wavefront(glrtx_group_ctx(grp_, i), 1) != GLRTX_OK) GLRT_FatalError("glrtx_set_texture_wavefront: %s", glrtx_last_error(glrtx_group_ctx(grp_, i)));
        GLRT_Info("texture wavefront: textured launches run on the wavefront kernel where they can");
    }
    uploadEnvironment();
    resize(scene->width, scene->height);
    if (const char *e = std::getenv("GLRT_BVH_ORDER")) orderByHits_ = std::string(e) == "hits";
    if (orderByHits_ && !scene->nodes.empty() && scene->textures_.empty() && scene->maps_.empty() && scene->cutouts_.empty() && scene->emissionMaps_.empty() && !scene->environment_.present && scene->spheres.empty() && !scene->hasDielectric_ && !scene->whitted_ && !scene->hasVolume_) {
        // one calibration frame on the first member's share of the rows (interleaved stripes: a fair sample of the image), counted by the render kernel itself
        glrtx_params p;
        frameParams(p);
        glrt_frame_seed(0x9e3779b9u, p.seed);
        std::vector<uint32_t> hist(scene->triangles.size(), 0u);
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_hit_histogram(c0, &p, hist.data(), hist.size()) != GLRTX_OK) GLRT_FatalError("glrtx_hit_histogram: %s", glrtx_last_error(c0));
        if (glrt_bvh_add_shadow_hits(hist.data(), hist.size(), &scene->triangles[0].indices[0], &scene->materials[0].type[0], scene->materials.size()) < 0)
            GLRT_FatalError("glrt_bvh_add_shadow_hits failed");
        const int exchanged = glrt_bvh_order_by_hits(&scene->nodes[0].bboxMin[0], scene->nodes.size(), hist.data(), hist.size());
        if (exchanged < 0) GLRT_FatalError("glrt_bvh_order_by_hits failed (%d)", exchanged);
        GLRT_Info("BVH: children ordered by the hits of a calibration frame, %d forks exchanged", exchanged);
        GLRTX_CHECK(glrtx_group_upload_scene(
            grp_, &scene->vertices[0].pos[0], scene->vertices.size(), &scene->triangles[0].indices[0], scene->triangles.size(),
            &scene->materials[0].type[0], scene->materials.size(), scene->lights.empty() ? nullptr : &scene->lights[0].indices[0], scene->lights.size(),
            &scene->nodes[0].bboxMin[0], scene->nodes.size()));
    }
    initialize();
    // The reference presents (and saves) every frame; when only the final image is wanted the frames of a static
    // camera go to the device several at a time -- same pixels, bit for bit, fewer and fuller launches.
    const bool every = saveEveryFrame_ && !output_.empty();
    const int step = every ? 1 : framesInFlight_;
    // Launches are issued back to back and the loop waits for the device only where it needs the pixels (a frame that is saved, the end of the run): the calls are
    // asynchronous, and a launch issued behind idle time runs longer -- 2 % behind 1 ms, 5 % behind 3 ms (profiles/r04_ab_launch_warmth.txt).  lastFrameMs() is the wall
    // time per frame between two such waits.
    if (bloom_ && (glrtx_group_size(grp_) != 1 || every)) GLRT_FatalError("--bloom: one device, and not with --save-every-frame (groups and the present ring have no bloomed form)");
    if (tonemap_ && (glrtx_group_size(grp_) != 1 || every)) GLRT_FatalError("--tonemap: one device, and not with --save-every-frame (groups and the present ring have no tone-mapped form)");
    if (!animationFile_.empty()) {
        animate();
        return;
    }
    if (denoise_ || denoiseVar_) {  // the feature planes of this (static) camera, once, before the first frame
        if (glrtx_group_size(grp_) != 1 || every) GLRT_FatalError("--denoise: one device, and not with --save-every-frame (groups and the present ring have no denoised form)");
        if (denoiseVar_ && (denoise_ || adaptive_)) GLRT_FatalError("--denoise-variance: not with --denoise or --adaptive");
        glrtx_params p;
        frameParams(p);
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_render_features(c0, &p) != GLRTX_OK) GLRT_FatalError("glrtx_render_features: %s", glrtx_last_error(c0));
    }
    auto t0 = std::chrono::steady_clock::now();
    if (every) {
        // The reference's cadence without its waits: every frame's image comes out of the ring the group presents into (glrtx_group_present_enable) -- resolved in the
        // pass that accumulates it and copied to pinned memory on a stream of its own -- so the frames are issued back to back and stay fed launches, and this thread
        // only waits when the ring is full.  Same PNG bytes and the same "Save:" line per frame as a sync + resolve per frame.
        GLRTX_CHECK(glrtx_group_present_enable(grp_, kPresentRing, 2.2f, 1));
        int images = 0;
        auto drain = [&](int wait) {
            glrtx_image img;
            int rc;
            while ((rc = glrtx_group_present_acquire(grp_, wait, &img)) == GLRTX_OK) {
                saveImage(output_, true, img.rgba);
                GLRTX_CHECK(glrtx_group_present_release(grp_, &img));
                images++;
                if (wait) break;  // (one is enough to free a ring image)
            }
            if (rc != GLRTX_OK && rc != GLRTX_EBUSY) GLRT_FatalError("glrtx_group_present_acquire: %s", glrtx_group_last_error(grp_));
        };
        // (images are taken only when the ring is full: a PNG written between two frames would let the running launch run dry, and the next frame would start a
        //  launch of its own instead of being appended to it)
        for (int i = 0; i < frameLimit_; i++) {
            if (i - images >= kPresentRing) drain(1);  // (a full ring would refuse the frame with GLRTX_EBUSY: one image out first)
            render();
        }
        while (images < frameLimit_) drain(1);
        GLRTX_CHECK(glrtx_group_sync(grp_));
        lastMs_ = frameLimit_ > 0 ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / frameLimit_ : 0.0;
        GLRTX_CHECK(glrtx_group_present_enable(grp_, 0, 2.2f, 1));
        glrtx_stats st;
        GLRTX_CHECK(glrtx_group_get_stats(grp_, &st));
        GLRT_Info("Presented: %d frames, %d images, %llu render kernel launches", frameLimit_, images, (unsigned long long)st.kernel_launches);
        return;
    }
    if (adaptiveVar_) {
        // Adaptive sampling by variance: --adaptive's bursts with every selection made from the moments plane, which the bursts themselves feed.
        if (glrtx_group_size(grp_) != 1 || adaptive_) GLRT_FatalError("--adaptive-variance: one device, and not with --adaptive (groups have no moments plane)");
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_track_moments(c0, 1) != GLRTX_OK) GLRT_FatalError("glrtx_track_moments: %s", glrtx_last_error(c0));
        glrtx_params p;
        frameParams(p);
        const glrtx_adaptive cfg = {adaptThreshold_, adaptMinSamples_};
        int issued = 0;
        while (issued < frameLimit_) {
            const int n = frameLimit_ - issued < framesInFlight_ ? frameLimit_ - issued : framesInFlight_;
            std::vector<float> seeds(2 * (size_t)n);
            for (int f = 0; f < n; f++) glrt_frame_seed(frame_++, &seeds[2 * (size_t)f]);
            if (glrtx_render_adaptive_moments(c0, &p, seeds.data(), n, &cfg) != GLRTX_OK) GLRT_FatalError("glrtx_render_adaptive_moments: %s", glrtx_last_error(c0));
            issued += n;
            int active = 0, total = 0;
            if (glrtx_adaptive_active_tiles(c0, &active, &total) != GLRTX_OK) GLRT_FatalError("glrtx_adaptive_active_tiles: %s", glrtx_last_error(c0));
            GLRT_Info("Adaptive: frame %d, active tiles %d/%d", issued, active, total);
            if (active == 0) break;
        }
        lastMs_ = issued > 0 ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / issued : 0.0;
        if (!output_.empty() && frameLimit_ > 0) saveCurrentFrame(output_, true);
        return;
    }
    if (denoiseVar_) {
        // Variance guidance: the frames in bursts of framesInFlight_ through glrtx_render_moments, which folds every sample into the moments plane as well.
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_track_moments(c0, 1) != GLRTX_OK) GLRT_FatalError("glrtx_track_moments: %s", glrtx_last_error(c0));
        glrtx_params p;
        frameParams(p);
        for (int issued = 0; issued < frameLimit_;) {
            const int n = frameLimit_ - issued < framesInFlight_ ? frameLimit_ - issued : framesInFlight_;
            std::vector<float> seeds(2 * (size_t)n);
            for (int f = 0; f < n; f++) glrt_frame_seed(frame_++, &seeds[2 * (size_t)f]);
            if (glrtx_render_moments(c0, &p, seeds.data(), n) != GLRTX_OK) GLRT_FatalError("glrtx_render_moments: %s", glrtx_last_error(c0));
            issued += n;
        }
        GLRTX_CHECK(glrtx_group_sync(grp_));
        lastMs_ = frameLimit_ > 0 ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / frameLimit_ : 0.0;
        if (!output_.empty() && frameLimit_ > 0) saveCurrentFrame(output_, true);
        return;
    }
    if (reweight_) {
        // Firefly re-weighting: the frames in bursts of framesInFlight_ through glrtx_render_cascades, which splits every sample over the cascade planes as well.
        if (glrtx_group_size(grp_) != 1 || denoise_ || denoiseVar_ || adaptive_) GLRT_FatalError("--reweight: one device, and not with --denoise, --denoise-variance or --adaptive*");
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_track_cascades(c0, 1, reweightStart_) != GLRTX_OK) GLRT_FatalError("glrtx_track_cascades: %s", glrtx_last_error(c0));
        glrtx_params p;
        frameParams(p);
        for (int issued = 0; issued < frameLimit_;) {
            const int n = frameLimit_ - issued < framesInFlight_ ? frameLimit_ - issued : framesInFlight_;
            std::vector<float> seeds(2 * (size_t)n);
            for (int f = 0; f < n; f++) glrt_frame_seed(frame_++, &seeds[2 * (size_t)f]);
            if (glrtx_render_cascades(c0, &p, seeds.data(), n) != GLRTX_OK) GLRT_FatalError("glrtx_render_cascades: %s", glrtx_last_error(c0));
            issued += n;
        }
        GLRTX_CHECK(glrtx_group_sync(grp_));
        lastMs_ = frameLimit_ > 0 ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / frameLimit_ : 0.0;
        if (!output_.empty() && frameLimit_ > 0) saveCurrentFrame(output_, true);
        return;
    }
    if (adaptive_) {
        // Adaptive sampling: every burst re-selects the tiles that are still active (from the accumulator as it stands) and renders its frames on those only; the
        // count the burst was issued on is reported after it.  A burst that found no active tile rendered nothing: the run ends there.
        glrtx_params p;
        frameParams(p);
        const glrtx_adaptive cfg = {adaptThreshold_, adaptMinSamples_};
        int issued = 0;
        while (issued < frameLimit_) {
            const int n = frameLimit_ - issued < framesInFlight_ ? frameLimit_ - issued : framesInFlight_;
            std::vector<float> seeds(2 * (size_t)n);
            for (int f = 0; f < n; f++) glrt_frame_seed(frame_++, &seeds[2 * (size_t)f]);
            GLRTX_CHECK(glrtx_group_render_adaptive(grp_, &p, seeds.data(), n, &cfg));
            issued += n;
            int active = 0, total = 0;
            GLRTX_CHECK(glrtx_group_adaptive_active_tiles(grp_, &active, &total));
            GLRT_Info("Adaptive: frame %d, active tiles %d/%d", issued, active, total);
            if (active == 0) break;
        }
        lastMs_ = issued > 0 ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / issued : 0.0;
        if (!output_.empty() && frameLimit_ > 0) saveCurrentFrame(output_, true);
        return;
    }
    int since = 0;
    for (int i = 0; i < frameLimit_; i += step) {
        const int n = frameLimit_ - i < step ? frameLimit_ - i : step;
        if (n == 1) render();
        else renderFrames(n);
        since += n;
        if (every || i + step >= frameLimit_) {
            GLRTX_CHECK(glrtx_group_sync(grp_));
            lastMs_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / since;
            if (every) saveCurrentFrame(output_, true);  // window.cpp:164
            t0 = std::chrono::steady_clock::now();
            since = 0;
        }
    }
    if (!every && !output_.empty() && frameLimit_ > 0) saveCurrentFrame(output_, true);
}

// --animate: the steps of the animation file, posed on the device (window.h: setAnimation has the call sequence).
void Window::animate() {
    if (glrtx_group_size(grp_) != 1) GLRT_FatalError("--animate: one device (groups have no pose call)");
    if (saveEveryFrame_) GLRT_FatalError("--animate: not with --save-every-frame (a step writes one image)");
    if (adaptive_ || adaptiveVar_) GLRT_FatalError("--animate: not with --adaptive or --adaptive-variance");
    if (reweight_) GLRT_FatalError("--animate: not with --reweight");
    if (scene->hasVolume_ || scene->volume_) GLRT_FatalError("--animate: not with --enable-volume (the volume does not move)");
    if (scene->extensions_ || !scene->spheres.empty() || scene->hasDielectric_ || scene->whitted_) GLRT_FatalError("--animate: not with --extensions (spheres do not move)");
    if (carryHistory_ && denoise_) GLRT_FatalError("--carry-history: not with --denoise (the fixed-sigma filter has no moments; use --denoise-variance)");
    if (denoise_ && denoiseVar_) GLRT_FatalError("--denoise-variance: not with --denoise");
    scene->parseAnimation(animationFile_);
    const std::vector<Scene::AnimationStep> &steps = scene->animation();
    const size_t n_vert = scene->vertices.size(), n_shapes = scene->numShapes();
    if (n_vert == 0 || n_shapes == 0 || n_shapes > 65536) GLRT_FatalError("--animate: the scene needs geometry and 1 .. 65536 shapes (it has %zu)", n_shapes);
    glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
    {  // the rig: the scene's vertices are the rest pose, vertex v follows the shape it came from alone
        std::vector<int32_t> bones(4 * n_vert, 0);
        std::vector<float> weights(4 * n_vert, 0.0f);
        for (size_t i = 0; i < n_shapes; i++)
            for (size_t v = scene->shapeFirstVertex(i); v < scene->shapeFirstVertex(i + 1); v++) { bones[4 * v] = (int32_t)i; weights[4 * v] = 1.0f; }
        if (glrtx_upload_rig(c0, &scene->vertices[0].pos[0], n_vert, bones.data(), weights.data(), (int)n_shapes) != GLRTX_OK)
            GLRT_FatalError("glrtx_upload_rig: %s", glrtx_last_error(c0));
    }
    const int n_targets = (int)scene->numMorphTargets();  // the file's morph targets go up after the rig; with them a step is a glrtx_pose_morph
    if (n_targets > 0 && scene->morphSparse()) {  // ("sparse_targets": true: the parser's index, never a dense array)
        if (glrtx_upload_morph_targets_sparse(c0, scene->morphOffsets().data(), scene->morphVertex().data(), scene->morphSparseDeltas().data(), n_targets, n_vert) !=
            GLRTX_OK)
            GLRT_FatalError("glrtx_upload_morph_targets_sparse: %s", glrtx_last_error(c0));
    } else if (n_targets > 0 && glrtx_upload_morph_targets(c0, scene->morphDeltas().data(), n_targets, n_vert) != GLRTX_OK)
        GLRT_FatalError("glrtx_upload_morph_targets: %s", glrtx_last_error(c0));
    if (scene->rebuildNormals()) {  // ("rebuild_normals": true: the topology of the rest pose beside the rig, and the switch before the first step)
        if (glrtx_upload_normal_topology(c0, &scene->vertices[0].pos[0], n_vert, &scene->triangles[0].indices[0], scene->triangles.size(),
                                         scene->normalTopologyFlags()) != GLRTX_OK)
            GLRT_FatalError("glrtx_upload_normal_topology: %s", glrtx_last_error(c0));
        if (glrtx_set_pose_normals(c0, 1) != GLRTX_OK) GLRT_FatalError("glrtx_set_pose_normals: %s", glrtx_last_error(c0));
    }
    float view0[16], proj0[16];
    std::memcpy(view0, scene->viewM, sizeof view0);
    std::memcpy(proj0, scene->projM, sizeof proj0);
    const float aperture0 = scene->apertureRadius, focal0 = scene->focalLength;
    const bool moments = carryHistory_ || denoiseVar_;
    const glrtx_reproject_cfg carry = {32, 0.02f, 0.9f};  // (glrt_amd.host.REPROJECT_DEFAULTS holds the same)
    const size_t dot = output_.find_last_of('.'), slash = output_.find_last_of("/\\");
    const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
    const std::string stem = has_ext ? output_.substr(0, dot) : output_, ext = has_ext ? output_.substr(dot) : "";
    for (size_t s = 0; s < steps.size(); s++) {
        const Scene::AnimationStep &st = steps[s];
        std::memcpy(scene->viewM, st.hasCamera ? st.viewM : view0, sizeof view0);
        std::memcpy(scene->projM, st.hasCamera ? st.projM : proj0, sizeof proj0);
        scene->apertureRadius = st.hasCamera ? st.apertureRadius : aperture0;
        scene->focalLength = st.hasCamera ? st.focalLength : focal0;
        auto t0 = std::chrono::steady_clock::now();
        if (n_targets > 0) {
            if (glrtx_pose_morph(c0, st.matrices.data(), (int)n_shapes, st.weights.data(), n_targets) != GLRTX_OK)
                GLRT_FatalError("glrtx_pose_morph: %s", glrtx_last_error(c0));
        } else if (glrtx_pose(c0, st.matrices.data(), (int)n_shapes) != GLRTX_OK) GLRT_FatalError("glrtx_pose: %s", glrtx_last_error(c0));
        glrtx_params p;
        frameParams(p);
        if (carryHistory_) {
            if (s == 0) {
                if (glrtx_track_motion(c0, 1) != GLRTX_OK) GLRT_FatalError("glrtx_track_motion: %s", glrtx_last_error(c0));
                if (glrtx_track_moments(c0, 1) != GLRTX_OK) GLRT_FatalError("glrtx_track_moments: %s", glrtx_last_error(c0));
                if (glrtx_render_features(c0, &p) != GLRTX_OK) GLRT_FatalError("glrtx_render_features: %s", glrtx_last_error(c0));
            } else {
                if (glrtx_reproject_motion(c0, &p, &carry) != GLRTX_OK) GLRT_FatalError("glrtx_reproject_motion: %s", glrtx_last_error(c0));
                int carried = 0, hits = 0;
                if (glrtx_reproject_last(c0, &carried, &hits) != GLRTX_OK) GLRT_FatalError("glrtx_reproject_last: %s", glrtx_last_error(c0));
                GLRT_Info("Animate: step %zu carries history at %d of %d hit pixels", s, carried, hits);
            }
        } else {
            GLRTX_CHECK(glrtx_group_clear(grp_));
            if ((denoise_ || denoiseVar_) && glrtx_render_features(c0, &p) != GLRTX_OK) GLRT_FatalError("glrtx_render_features: %s", glrtx_last_error(c0));
            if (denoiseVar_ && s == 0 && glrtx_track_moments(c0, 1) != GLRTX_OK) GLRT_FatalError("glrtx_track_moments: %s", glrtx_last_error(c0));
        }
        for (int issued = 0; issued < frameLimit_;) {
            const int n = frameLimit_ - issued < framesInFlight_ ? frameLimit_ - issued : framesInFlight_;
            if (moments) {
                std::vector<float> seeds(2 * (size_t)n);
                for (int f = 0; f < n; f++) glrt_frame_seed(frame_++, &seeds[2 * (size_t)f]);
                if (glrtx_render_moments(c0, &p, seeds.data(), n) != GLRTX_OK) GLRT_FatalError("glrtx_render_moments: %s", glrtx_last_error(c0));
            } else if (n == 1) render();
            else renderFrames(n);
            issued += n;
        }
        GLRTX_CHECK(glrtx_group_sync(grp_));
        lastMs_ = frameLimit_ > 0 ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / frameLimit_ : 0.0;
        char num[16];
        std::snprintf(num, sizeof num, "_%04zu", s);
        if (!output_.empty()) saveCurrentFrame(stem + num + ext, true);
    }
    std::memcpy(scene->viewM, view0, sizeof view0);
    std::memcpy(scene->projM, proj0, sizeof proj0);
    scene->apertureRadius = aperture0; scene->focalLength = focal0;
}

void Window::initialize() {
    for (int i = 0; i < glrtx_group_size(grp_); i++)
        if (glrtx_count_rays(glrtx_group_ctx(grp_, i), 1) != GLRTX_OK) GLRT_FatalError("glrtx_count_rays failed");
}

void Window::frameParams(glrtx_params &p) const {
    // window.cpp:230-243: the per-frame uniforms (u_seed is filled in by the caller)
    float cam[16];
    glrt_mat4_mul(scene->viewM, scene->modelM, cam);
    if (glrt_mat4_inverse(cam, p.c2w) != GLRT_HOST_OK || glrt_mat4_inverse(scene->projM, p.s2c) != GLRT_HOST_OK)
        GLRT_FatalError("camera matrix is singular");
    p.aperture = scene->apertureRadius;
    p.focal = scene->focalLength;
    p.seed[0] = p.seed[1] = 0.0f;
    p.n_samples = samplesPerFrame_;
    p.max_depth = maxDepth_;
}

void Window::render() {
    glrtx_params p;
    frameParams(p);
    glrt_frame_seed(frame_++, p.seed);
    GLRTX_CHECK(glrtx_group_render(grp_, &p));  // window.cpp:290, the draw that runs the path tracer
    noteFallback();
}

// Once per run: say so when launches leave the wavefront kernel for the (slower) persistent megakernel (glrtx_stats.fallback_last).
void Window::noteFallback() {
    if (fallbackNoted_) return;
    glrtx_stats st;
    if (glrtx_group_get_stats(grp_, &st) != GLRTX_OK || st.fallback_launches == 0) return;
    fallbackNoted_ = true;
    GLRT_Info("Render kernel: persistent megakernel instead of the wavefront kernel (%s%s%s): about half the rays per second, no frames in flight",
              (st.fallback_last & GLRTX_FALLBACK_DEPTH) ? "u_maxDepth > 255 " : "", (st.fallback_last & GLRTX_FALLBACK_SAMPLES) ? "u_nSamples >= 2^20 " : "",
              (st.fallback_last & GLRTX_FALLBACK_EXTENSIONS) ? "extension scene" : "");
}

void Window::renderFrames(int n) {
    glrtx_params p;
    frameParams(p);
    std::vector<float> seeds(2 * (size_t)n);
    for (int f = 0; f < n; f++) glrt_frame_seed(frame_++, &seeds[2 * (size_t)f]);
    GLRTX_CHECK(glrtx_group_render_frames(grp_, &p, seeds.data(), n));
    noteFallback();
}

void Window::resizeDefault(int w, int h) {
    width_ = w;
    height_ = h;
    resetBuffer();
}

void Window::resetBuffer() { GLRTX_CHECK(glrtx_group_resize(grp_, width_, height_)); }  // window.cpp:366-381

void Window::saveCurrentFrame(const std::string &filename, bool overwrite) const {
    std::vector<unsigned char> bytes((size_t)width_ * height_ * 4);
    if (tonemap_ || bloom_) {  // --tonemap / --bloom: the denoised image if one was asked for, else the accumulator, through the exposure and the tone curve (one device: checked in mainloop)
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        glrtx_tonemap_cfg cfg = tonemapCfg_;
        cfg.source = (denoise_ || denoiseVar_ || reweight_) ? 1 : 0;
        if (reweight_) {
            if (glrtx_reweight(c0, &reweightCfg_) != GLRTX_OK) GLRT_FatalError("glrtx_reweight: %s", glrtx_last_error(c0));
            GLRT_Info("Reweight: kappa %g, start %g", (double)reweightCfg_.kappa, (double)reweightStart_);
        }
        if (denoise_ && glrtx_denoise(c0, &denoiseCfg_) != GLRTX_OK) GLRT_FatalError("glrtx_denoise: %s", glrtx_last_error(c0));
        if (denoiseVar_ && glrtx_denoise_variance(c0, &denoiseVarCfg_) != GLRTX_OK) GLRT_FatalError("glrtx_denoise_variance: %s", glrtx_last_error(c0));
        if (cfg.auto_exposure && glrtx_exposure_measure(c0, &cfg) != GLRTX_OK) GLRT_FatalError("glrtx_exposure_measure: %s", glrtx_last_error(c0));
        if (bloom_) {  // the glow on the linear image, then the curve (op 0 at exposure 1 without --tonemap) over B; the exposure was measured on the unbloomed source
            glrtx_bloom_cfg bc = bloomCfg_;
            bc.source = cfg.source;
            if (glrtx_bloom(c0, &bc) != GLRTX_OK) GLRT_FatalError("glrtx_bloom: %s", glrtx_last_error(c0));
            if (glrtx_resolve_bloomed_rgba8(c0, bytes.data(), (size_t)width_ * 4, &cfg) != GLRTX_OK) GLRT_FatalError("glrtx_resolve_bloomed_rgba8: %s", glrtx_last_error(c0));
            GLRT_Info("Bloom: threshold %g, strength %g, %d levels", (double)bc.threshold, (double)bc.strength, bc.levels);
        } else if (glrtx_resolve_tonemapped_rgba8(c0, bytes.data(), (size_t)width_ * 4, &cfg) != GLRTX_OK)
            GLRT_FatalError("glrtx_resolve_tonemapped_rgba8: %s", glrtx_last_error(c0));
        if (cfg.auto_exposure) {
            glrtx_exposure e;
            if (glrtx_read_exposure(c0, &e) != GLRTX_OK) GLRT_FatalError("glrtx_read_exposure: %s", glrtx_last_error(c0));
            GLRT_Info("Tonemap: op %d, exposure %g x measured %g (mean log2 luminance %g over %llu of %llu pixels)", cfg.op, (double)cfg.exposure, (double)e.exposure,
                      (double)e.mean_log2, (unsigned long long)e.kept, (unsigned long long)e.counted);
        } else
            GLRT_Info("Tonemap: op %d, exposure %g", cfg.op, (double)cfg.exposure);
        saveImage(filename, overwrite, bytes.data());
        return;
    }
    // resolve = screen.frag (rgb/count, clamp, gamma 2.2) + the vertical flip of window.cpp:391-398
    // (with several GPUs the stripes are first gathered on the first one)
    if (denoise_) {  // the filter's result through the same resolve
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_denoise(c0, &denoiseCfg_) != GLRTX_OK || glrtx_resolve_denoised_rgba8(c0, bytes.data(), (size_t)width_ * 4, 2.2f, 1) != GLRTX_OK)
            GLRT_FatalError("glrtx_denoise: %s", glrtx_last_error(c0));
        GLRT_Info("Denoise: %d iterations", denoiseCfg_.iterations);
    } else if (denoiseVar_) {
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_denoise_variance(c0, &denoiseVarCfg_) != GLRTX_OK || glrtx_resolve_denoised_rgba8(c0, bytes.data(), (size_t)width_ * 4, 2.2f, 1) != GLRTX_OK)
            GLRT_FatalError("glrtx_denoise_variance: %s", glrtx_last_error(c0));
        GLRT_Info("Denoise (variance-guided): %d iterations", denoiseVarCfg_.iterations);
    } else if (reweight_) {  // the re-weighted image through the same resolve
        glrtx_ctx *c0 = glrtx_group_ctx(grp_, 0);
        if (glrtx_reweight(c0, &reweightCfg_) != GLRTX_OK || glrtx_resolve_denoised_rgba8(c0, bytes.data(), (size_t)width_ * 4, 2.2f, 1) != GLRTX_OK)
            GLRT_FatalError("glrtx_reweight: %s", glrtx_last_error(c0));
        GLRT_Info("Reweight: kappa %g, start %g", (double)reweightCfg_.kappa, (double)reweightStart_);
    } else if (glrtx_group_resolve_rgba8(grp_, bytes.data(), (size_t)width_ * 4, 2.2f, 1) != GLRTX_OK)
        GLRT_FatalError("glrtx_group_resolve_rgba8: %s", glrtx_group_last_error(grp_));
    saveImage(filename, overwrite, bytes.data());
}

void Window::saveImage(const std::string &filename, bool overwrite, const unsigned char *bytes) const {
    std::string path = filename;
    if (!overwrite) {
        int count = 0;
        const size_t dot = filename.find_last_of('.');
        const std::string base = filename.substr(0, dot), ext = dot == std::string::npos ? "" : filename.substr(dot);
        while (std::ifstream(path).good()) path = base + "_" + std::to_string(count++) + ext;
    }
    if (!writePng(path, width_, height_, bytes)) GLRT_Warn("Failed to save: %s", path.c_str());
    else GLRT_Info("Save: %s", path.c_str());
}

// ---------------------------------------------------------------------------------------------- PNG
namespace {
uint32_t crc32(const unsigned char *d, size_t n, uint32_t c = 0) {
    static uint32_t table[256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t r = i;
            for (int k = 0; k < 8; k++) r = (r & 1) ? 0xEDB88320u ^ (r >> 1) : r >> 1;
            table[i] = r;
        }
        init = true;
    }
    c = ~c;
    for (size_t i = 0; i < n; i++) c = table[(c ^ d[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}
void be32(std::vector<unsigned char> &v, uint32_t x) {
    v.push_back((unsigned char)(x >> 24)); v.push_back((unsigned char)(x >> 16));
    v.push_back((unsigned char)(x >> 8)); v.push_back((unsigned char)x);
}
void chunk(std::vector<unsigned char> &out, const char *type, const std::vector<unsigned char> &data) {
    be32(out, (uint32_t)data.size());
    std::vector<unsigned char> td(type, type + 4);
    td.insert(td.end(), data.begin(), data.end());
    out.insert(out.end(), td.begin(), td.end());
    be32(out, crc32(td.data(), td.size()));
}
}  // namespace

bool writePng(const std::string &filename, int w, int h, const unsigned char *rgba) {
    std::vector<unsigned char> raw;
    raw.reserve((size_t)h * ((size_t)w * 4 + 1));
    for (int y = 0; y < h; y++) {
        raw.push_back(0);  // filter: none
        raw.insert(raw.end(), rgba + (size_t)y * w * 4, rgba + (size_t)(y + 1) * w * 4);
    }
    std::vector<unsigned char> z = {0x78, 0x01};  // zlib header, stored blocks
    uint32_t a = 1, b = 0;
    for (unsigned char c : raw) { a = (a + c) % 65521u; b = (b + a) % 65521u; }
    for (size_t off = 0; off < raw.size() || off == 0; off += 65535) {
        const size_t n = std::min<size_t>(65535, raw.size() - off);
        z.push_back(off + n >= raw.size() ? 1 : 0);
        z.push_back((unsigned char)(n & 0xFF)); z.push_back((unsigned char)(n >> 8));
        z.push_back((unsigned char)(~n & 0xFF)); z.push_back((unsigned char)((~n >> 8) & 0xFF));
        z.insert(z.end(), raw.begin() + (long)off, raw.begin() + (long)(off + n));
        if (raw.empty()) break;
    }
    be32(z, (b << 16) | a);
    std::vector<unsigned char> png = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::vector<unsigned char> ihdr;
    be32(ihdr, (uint32_t)w); be32(ihdr, (uint32_t)h);
    ihdr.insert(ihdr.end(), {8, 6, 0, 0, 0});  // 8-bit RGBA
    chunk(png, "IHDR", ihdr);
    chunk(png, "IDAT", z);
    chunk(png, "IEND", {});
    std::ofstream f(filename.c_str(), std::ios::binary);
    if (f.fail()) return false;
    f.write((const char *)png.data(), (std::streamsize)png.size());
    return f.good();
}

}  // namespace glrt
