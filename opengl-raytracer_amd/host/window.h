// window.h -- glrt::Window, the drop-in render-loop class (reference: src/core/window.h:14-58).
// Same public surface -- Window(), mainloop(scene, fps = -1), width(), height() -- and the same
// protected virtual hooks (initialize/render/resize/mouse/keyboard), but headless: no GLFW window,
// no GL context, no ImGui.  render() forwards to the C-ABI HIP layer (include/glrtx.h) where the
// reference's render() issued GL calls (window.cpp:213-318).  Because nothing ever closes a headless
// window, the loop runs for a fixed number of frames (setFrameLimit / GLRT_FRAMES, default 16).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "glrtx.h"
#include "scene.h"

struct glrtx_group;
struct glrtx_params;

namespace glrt {

struct MouseEvent { int button = 0, action = 0, mods = 0; double x = 0, y = 0; };  // event.h stand-in (never raised)

class GLRT_API Window {
public:
    Window();
    virtual ~Window();
    void mainloop(const std::shared_ptr<Scene> &scene, double fps = -1.0);
    int width() const { return width_; }
    int height() const { return height_; }

    // Headless controls (the reference hard-codes these: u_nSamples = 1 at window.cpp:239, u_maxDepth
    // left at the shader default 16, a fresh random u_seed per frame at :226-238, output.png every frame).
    void setFrameLimit(int frames) { frameLimit_ = frames; }
    void setMaxDepth(int depth) { maxDepth_ = depth; }
    void setSamplesPerFrame(int spp) { samplesPerFrame_ = spp; }
    void setOutput(const std::string &file, bool everyFrame = false) { output_ = file; saveEveryFrame_ = everyFrame; }
    void setDevice(int hipDevice) { devices_.assign(1, hipDevice); }
    // Several GPUs of the node (no reference counterpart): the image rows are split into interleaved 8-row stripes, one share per
    // listed HIP device, rendered concurrently and gathered on the first one when a frame is saved (glrtx_group, include/glrtx.h).
    // The same ordinal may be listed more than once.  The image is bit-identical to the single-GPU one.  GLRT_GPUS=N = devices 0..N-1.
    void setDevices(const std::vector<int> &hipDevices) { if (!hipDevices.empty()) devices_ = hipDevices; }
    void setFirstFrame(unsigned f) { frame_ = f; }
    // Profile-guided child order (no reference counterpart; off by default; GLRT_BVH_ORDER=hits): before the first frame one calibration frame of the scene's camera is
    // rendered, the closest hits per triangle are counted by the render kernel (glrtx_hit_histogram) and at every fork of the BVH the child that is hit more often goes
    // into the slot the traversal visits first (glrt_bvh_order_by_hits): config 5 -1 %, config 4 -1.8 %, the Cornell-box scenes +-0.3 % (profiles/r06_hit_order.txt).
    // Exact ties between two triangles may resolve to the other one.
    void setOrderChildrenByHits(bool on) { orderByHits_ = on; }
    // Frames issued per launch of the render kernel (glrtx_render_frames; bit-identical to one launch per frame).
    // Used when no image is written between frames and render() is not overridden per frame; GLRT_FRAMES_IN_FLIGHT.
    void setFramesInFlight(int n) { framesInFlight_ = n < 1 ? 1 : n; }
    // Adaptive sampling (no reference counterpart; glrtx_render_adaptive): bursts of framesInFlight frames, each on the 8x8 tiles that have not converged
    // (error above threshold, or fewer than minSamples samples), until no tile is active or the frame limit is reached; one "Adaptive:" line per burst.
    void setAdaptive(float threshold, int minSamples) { adaptive_ = true; adaptThreshold_ = threshold; adaptMinSamples_ = minSamples; }
    // The same bursts with the selection made from the luminance moments (glrtx_render_adaptive_moments; tracking is switched on): one device; composes with
    // setDenoiseVariance, whose filter reads the variance the bursts fed.  Its thresholds are not setAdaptive's.
    void setAdaptiveVariance(float threshold, int minSamples) { adaptiveVar_ = true; adaptThreshold_ = threshold; adaptMinSamples_ = minSamples; }
    // Volume scenes on the wavefront kernel (glrtx_set_volume_wavefront on every member): frames in flight, fed launches and adaptive sampling with the volume
    // on; same images as the persistent megakernel, the default.  Adaptive sampling of a volume scene turns it on by itself.
    void setVolumeWavefront(bool on) { volumeWavefront_ = on; }
    // Textured scenes on the wavefront kernel (glrtx_set_texture_wavefront on every member): frames in flight and fed launches with textures and material maps
    // bound; same images as the textured megakernel, the default.  A scene the wavefront kernel cannot take (spheres, dielectric, an environment) renders as before.
    void setTextureWavefront(bool on) { textureWavefront_ = on; }
    // Denoising (no reference counterpart; glrtx_render_features / glrtx_denoise, one device only): the feature planes are rendered once before the first frame, and
    // every image that is written is the a-trous filter's result D instead of the raw mean.  iterations < 1: the default.
    void setDenoise(int iterations) { denoise_ = true; if (iterations >= 1) denoiseCfg_.iterations = iterations; }
    // Variance-guided denoising (glrtx_track_moments / glrtx_render_moments / glrtx_denoise_variance, one device only): the frames are rendered in bursts of
    // framesInFlight frames with the moments fold, and the saved image is the variance-guided filter's.
    // Tone mapping of the saved image (glrtx_exposure_measure / glrtx_resolve_tonemapped_rgba8, one device only): op 0 clamp, 1 Reinhard, 2 ACES; the source is the
    // denoised image when a denoiser is on.  Without it the saved image is the plain resolve's, byte for byte.
    void setTonemap(int op, float exposure, bool autoExposure) { tonemap_ = true; tonemapCfg_.op = op; tonemapCfg_.exposure = exposure; tonemapCfg_.auto_exposure = autoExposure ? 1 : 0; }
    // Bloom in front of the curve (glrtx_bloom / glrtx_resolve_bloomed_rgba8, one device only): the saved image is B -- the denoised image when a denoiser is on,
    // else the accumulator, plus the glow -- through the tone curve (clamp at exposure 1 without setTonemap).  Without it the saved image is what it was.
    void setBloom(float threshold, float strength, int levels) { bloom_ = true; bloomCfg_.threshold = threshold; bloomCfg_.strength = strength; bloomCfg_.levels = levels; }
    // Firefly re-weighting (glrtx_track_cascades / glrtx_render_cascades / glrtx_reweight, one device only): the frames are rendered in bursts of framesInFlight
    // frames with the cascade fold, and the saved image is the re-weighted one (through setBloom / setTonemap as a denoised image would go).
    void setReweight(float kappa, float start) { reweight_ = true; reweightCfg_.kappa = kappa; reweightStart_ = start; }
    void setDenoiseVariance(int iterations) { denoiseVar_ = true; if (iterations >= 1) denoiseVarCfg_.iterations = iterations; }
    // Animation (no reference counterpart; glrtx_upload_rig / glrtx_pose, one device only): the steps of `file` (Scene::parseAnimation has the format) are posed on
    // the device one after the other -- bone i is shape i of the scene file --, each rendered with the frame limit's frames and written to <stem>_<step, four
    // digits>.<ext> exactly as a still run writes its image under the same denoise / bloom / tonemap settings.  The frame counter behind the seeds runs on across
    // the steps.  Step s issues: glrtx_pose; then, with carryHistory, at s = 0 glrtx_track_motion(1), glrtx_track_moments(1) and glrtx_render_features, from
    // s = 1 on glrtx_reproject_motion with the default configuration -- without it glrtx_clear and the feature pass a still run's denoiser would make --; then the
    // frames in bursts of framesInFlight (through glrtx_render_moments when moments are tracked: carryHistory or setDenoiseVariance); then the image.
    // Not with several devices, setAdaptive*, setReweight, extension or volume scenes, one image per frame, or carryHistory with setDenoise (no moments).
    // A file with morph targets: glrtx_upload_morph_targets once after glrtx_upload_rig -- glrtx_upload_morph_targets_sparse for a file with "sparse_targets":
    // true --, and every step's pose is glrtx_pose_morph with the step's weights.  A file with "rebuild_normals": true: glrtx_upload_normal_topology of the
    // scene's vertices and triangles after them, then glrtx_set_pose_normals(1), so that every step's pose rebuilds the normals in front of its refit.
    void setAnimation(const std::string &file, bool carryHistory) { animationFile_ = file; carryHistory_ = carryHistory; }
    // wall-clock ms PER FRAME between the last two waits for the device, averaged over the frames issued in between (with one PNG per run: the whole run, cold first
    // launches included; with --save-every-frame: the whole run, PNG writing included).  The device's own time of the last launch is glrtx_stats.kernel_ms_last.
    double lastFrameMs() const { return lastMs_; }
    unsigned long long raysTraced() const;

protected:
    virtual void initialize();
    virtual void render();
    virtual void renderFrames(int n);  // n consecutive frames with a static camera, one launch
    virtual void resize(int width, int height) { resizeDefault(width, height); }
    virtual void mouse(const MouseEvent &) {}
    virtual void keyboard(int, int, int, int) {}

private:
    void frameParams(struct ::glrtx_params &p) const;
    void uploadTextures();  // the scene's texture set, then its material maps, on every member (glrtx_upload_textures, glrtx_bind_material_maps)
    void uploadEnvironment();  // the scene's environment on every member (glrtx_upload_environment)
    void resizeDefault(int width, int height);
    void resetBuffer();
    void saveCurrentFrame(const std::string &filename, bool overwrite = true) const;
    void saveImage(const std::string &filename, bool overwrite, const unsigned char *rgba) const;  // a full RGBA8 image, flipped: PNG + "Save:" line
    static constexpr int kPresentRing = 8;  // --save-every-frame: images the loop may run ahead of the PNG writer (8.3 MB each at 1080p, pinned)
    void noteFallback();
    void animate();

    glrtx_group *grp_ = nullptr;
    std::vector<int> devices_ = {-1};  // -1: the current HIP device
    int width_ = 0, height_ = 0;
    int frameLimit_ = 16, maxDepth_ = 16, samplesPerFrame_ = 1, framesInFlight_ = 16;
    unsigned frame_ = 0;
    bool saveEveryFrame_ = false;
    bool orderByHits_ = false;
    bool adaptive_ = false, adaptiveVar_ = false;
    float adaptThreshold_ = 0.0f;
    int adaptMinSamples_ = 2;
    bool volumeWavefront_ = false;
    bool textureWavefront_ = false;
    bool denoise_ = false, denoiseVar_ = false;
    bool reweight_ = false;
    glrtx_reweight_cfg reweightCfg_ = {4.0f};  // (glrt_amd.host.REWEIGHT_DEFAULTS holds the same)
    float reweightStart_ = 1.0f;
    bool tonemap_ = false;
    bool bloom_ = false;
    glrtx_bloom_cfg bloomCfg_ = {0, 1.0f, 0.25f, 5};  // (glrt_amd.host.BLOOM_DEFAULTS holds the same)
    glrtx_tonemap_cfg tonemapCfg_ = {0, 0, 0, 1.0f, 0.18f, 500, 950, 1.0f, 4.0f, 2.2f, 1};  // (glrt_amd.host.TONEMAP_DEFAULTS holds the same)
    glrtx_denoise_var_cfg denoiseVarCfg_ = {5, 4.0f, 0.1f, 0.01f, 1};  // (DESIGN.md "Variance guidance": the sweep; glrt_amd.host.DENOISE_VAR_DEFAULTS holds the same)
    glrtx_denoise_cfg denoiseCfg_ = {5, 100.0f, 0.1f, 0.01f, 1};  // (DESIGN.md "Denoising": the sweep behind these; glrt_amd.host.DENOISE_DEFAULTS holds the same)
    bool fallbackNoted_ = false;
    std::string animationFile_;
    bool carryHistory_ = false;
    std::string output_ = "output.png";
    double lastMs_ = 0.0;
    std::shared_ptr<Scene> scene = nullptr;
};

// RGBA8 -> PNG (stored deflate blocks; own encoder, the reference uses stb_image_write).
bool writePng(const std::string &filename, int w, int h, const unsigned char *rgba);

}  // namespace glrt
