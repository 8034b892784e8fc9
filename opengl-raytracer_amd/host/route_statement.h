// route_statement.h -- a launch's route (DESIGN.md "A launch's route"): which kernel a render call of a context runs, in which shading form, what the
// statistics report about it -- or why the call refuses -- as one pure function of the few context fields and parameters that decide it.  Stated once for the
// device layer (csrc/glrtx.hip: route_of) and the host library (host/route.cpp: glrt_launch_route).  Internal to the two libraries.
// tests/golden/route_matrix.txt pins it over every state (tests/test_route_host.py).
#pragma once
#include <cstdio>
#include <string>

namespace glrt_detail {

// The ranges of the wavefront kernel's packed path state (pt_kernel.hip.h) and the flag values of include/glrtx.h; csrc/glrtx.hip ties them to the originals.
constexpr int kWfDepthMax = 255, kWfSampleMax = (1 << 20) - 1, kWfVolSampleMax = (1 << 16) - 1;
constexpr int kRouteExtVolume = 4;                                                                // GLRTX_EXT_VOLUME
constexpr int kRouteFallbackDepth = 1, kRouteFallbackSamples = 2, kRouteFallbackExtensions = 4;  // GLRTX_FALLBACK_*

// What decides.  The two switches arrive resolved: glrtx_set_*_wavefront's value, or the override of GLRTX_VOLUME_WAVEFRONT / GLRTX_TEXTURE_WAVEFRONT.
struct RouteState {
    int variant, ext_flags, n_spheres, n_tex, n_vine;
    bool have_volume, have_maps, have_cut, have_emit, have_env, vol_switch, tex_switch;
    int max_depth, n_samples;
};

// The request, as RenderReq::Kind (csrc/glrtx.hip).  Moments, AdaptiveMoments and Cascades refuse the same list; Calibration is glrtx_hit_histogram.
enum RouteKind { kRouteOrdinary, kRouteAdaptive, kRouteMoments, kRouteCalibration, kRouteAdaptiveMoments, kRouteCascades, kRouteKinds };
enum RouteFamily { kRouteTile = 0, kRoutePersistent = 1, kRouteWavefront = 2 };  // the kernel family: glrtx_stats.variant_last

// The wavefront kernel's shading forms: rows of kWgwfNames.  (Fetch, compact layout and the tree's kind are wgwf_kernel's: they depend on sizes, not on what is bound.)
enum WgwfForm { kWfListScan, kWfTree, kWfVolume, kWfTex, kWfTexMaps, kWgwfForms };
constexpr const char *kWgwfNames[kWgwfForms][2] = {  // [form][adaptive] (error reports)
    {"pt_render_wgwf (list scan)", "pt_render_wgwf (adaptive, list scan)"}, {"pt_render_wgwf", "pt_render_wgwf (adaptive)"}, {"pt_render_wgwf (volume)", "pt_render_wgwf (volume, adaptive)"},
    {"pt_render_wgwf (textures)", "pt_render_wgwf (textures, adaptive)"}, {"pt_render_wgwf (textures, maps)", "pt_render_wgwf (textures, maps, adaptive)"}};

// The persistent megakernel's forms: rows of csrc/glrtx.hip's kPersistent, in this order.
enum PersistForm { kFormPlain, kFormExt, kFormVol, kFormTex, kFormTexVol, kFormTexMaps, kFormTexVolMaps, kFormEnv, kFormEnvTex, kFormEnvTexMaps,
                   kFormTexCut, kFormTexMapsCut, kFormEnvTexCut, kFormEnvTexMapsCut, kFormTexEmit, kFormTexMapsEmit, kFormEnvTexEmit, kFormEnvTexMapsEmit,
                   kPersistForms };
constexpr const char *kPersistentNames[kPersistForms] = {  // (error reports)
    "pt_render_persistent", "pt_render_persistent (extensions)", "pt_render_persistent (volume)", "pt_render_persistent (extensions, textures)",
    "pt_render_persistent (volume, textures)", "pt_render_persistent (extensions, textures, maps)", "pt_render_persistent (volume, textures, maps)",
    "pt_render_persistent (extensions, environment)", "pt_render_persistent (extensions, environment, textures)",
    "pt_render_persistent (extensions, environment, textures, maps)",
    "pt_render_persistent (extensions, textures, cutouts)", "pt_render_persistent (extensions, textures, maps, cutouts)",
    "pt_render_persistent (extensions, environment, textures, cutouts)", "pt_render_persistent (extensions, environment, textures, maps, cutouts)",
    "pt_render_persistent (extensions, textures, emission maps)", "pt_render_persistent (extensions, textures, maps, emission maps)",
    "pt_render_persistent (extensions, environment, textures, emission maps)", "pt_render_persistent (extensions, environment, textures, maps, emission maps)"};

struct Route {
    std::string refusal;   // "": the call launches; otherwise what it says behind "<function>: ", and nothing below counts
    int family, fallback;  // RouteFamily; glrtx_stats.fallback_last
    bool fallback_counts;  // whether the launch counts in fallback_launches: variant 2 is selected and another kernel runs
    int form;              // wavefront: WgwfForm; persistent: PersistForm; tile: 0
    const char *kernel;    // the form's name (error reports, glrtx_debug_last_kernel)
    bool vol, env, cut, emit, tex, maps, ext, vine;  // what the form is given.  wavefront: vol, tex, maps, vine; persistent: all but vine (ext: the extension kernel, with the spheres)
};

inline Route launch_route(const RouteState &s, RouteKind kind) {
    Route r{};
    char buf[160];
    const bool tex = s.n_tex > 0, adaptive = kind == kRouteAdaptive || kind == kRouteAdaptiveMoments;
    const bool deep = s.max_depth > kWfDepthMax;
    const bool holds = !deep && s.n_samples <= kWfSampleMax;  // the packed path state: meta = depth | sample << 8 | flags << 28 ...
    // The volume on the wavefront kernel's V form: the switch is on, the volume is the only extension, one is uploaded, and nothing else needs the megakernel.
    const bool vol_wf = s.vol_switch && s.ext_flags == kRouteExtVolume && s.have_volume && s.n_spheres == 0 && !tex && !s.have_env;
    const int sample_max = vol_wf ? kWfVolSampleMax : kWfSampleMax;  // ... the V form: sample in bits 8-23
    // A bound set on the wavefront kernel's T / TM forms: the first of these that keeps it off them
    const char *const tex_off = !tex ? "no set is bound"
                                : s.have_cut ? "cutouts are bound (the wavefront kernel's traversal step has no cutout form)"
                                : s.have_emit ? "emission maps are bound (the wavefront kernel's shade phase has no emission-map form)"
                                : !s.tex_switch ? "the texture wavefront switch is off (glrtx_set_texture_wavefront)"
                                : s.ext_flags != 0 ? "extensions or volume are on"
                                : s.n_spheres > 0 ? "spheres are uploaded"
                                : s.have_env ? "an environment is bound"
                                : s.n_vine > 0 ? "the tree is a vine (the list scan has no textured form)"
                                : nullptr;

    // ---- what only the wavefront kernel can do: the calls with a tile list or a side plane, and the calibration frame
    if (kind == kRouteCalibration) {
        r.refusal = tex && s.have_cut ? "textures are bound and cutouts are bound (wavefront kernel only)"
                    : tex && s.have_emit ? "textures are bound and emission maps are bound (wavefront kernel only)"
                    : tex ? "textures are bound (wavefront kernel only)"
                    : s.have_env ? "an environment is bound (wavefront kernel only)"
                    : s.variant != 2 || !holds || s.n_spheres > 0 || s.ext_flags != 0 ? "wavefront kernel only" : "";
    } else if (kind != kRouteOrdinary) {
        const bool tiles = kind == kRouteAdaptive;  // glrtx_render_adaptive: the tile list, and the V form; the others: the sample planes
        const char *const tex_why = !tex ? nullptr : tex_off ? tex_off : s.variant != 2 ? "the context's variant is not 2"
                                    : !holds ? "max_depth / n_samples beyond the wavefront kernel's path state" : nullptr;
        if (tex_why)
            r.refusal = std::string("textures are bound and the wavefront kernel does not shade them here: ") + tex_why +
                        (tiles ? " (only the wavefront kernel has a tile list)" : " (the megakernel that shades them writes no sample planes)");
        else if (s.ext_flags != 0 && !(tiles && vol_wf)) r.refusal = tiles ? "extensions or volume are on (only the wavefront kernel has a tile list)" : "extensions or volume are on";
        else if (s.n_spheres > 0) r.refusal = tiles ? "spheres are uploaded (only the wavefront kernel has a tile list)" : "spheres are uploaded";
        else if (s.have_env)
            r.refusal = tiles ? "an environment is bound (only the wavefront kernel has a tile list)" : "an environment is bound (the megakernel that shades it writes no sample planes)";
        else if (s.variant != 2 || deep || s.n_samples > sample_max) {  // (past the line above the V form is adaptive's alone)
            if (s.variant != 2) std::snprintf(buf, sizeof buf, "variant %d (only the wavefront kernel, variant 2, %s)", s.variant, tiles ? "has a tile list" : "writes sample planes");
            else std::snprintf(buf, sizeof buf, "max_depth %d / n_samples %d beyond the wavefront kernel's path state", s.max_depth, s.n_samples);
            r.refusal = buf;
        }
    }
    if (!r.refusal.empty()) return r;

    // ---- what no kernel renders beside the volume
    const bool volume = (s.ext_flags & kRouteExtVolume) != 0;
    if (volume)
        r.refusal = !s.have_volume ? "GLRTX_EXT_VOLUME is set and no volume is uploaded (glrtx_upload_volume)"
                    : s.have_env ? "GLRTX_EXT_VOLUME is set and an environment is bound (the volume branch has its own escape path)"
                    : tex && s.have_cut ? "GLRTX_EXT_VOLUME is set and cutouts are bound (the volume kernels have no cutout form)"
                    : tex && s.have_emit ? "GLRTX_EXT_VOLUME is set and emission maps are bound (the volume kernels have no emission-map form)" : "";
    if (!r.refusal.empty()) return r;

    // ---- the family.  The wavefront kernel (variant 2) takes a launch without extensions, or the volume alone on its V form, or a texture set alone on
    // its T / TM forms, within the range of its path state; the extension megakernel whatever else is bound; the selected variant the rest.
    const bool wavefront = s.variant == 2 && s.n_spheres == 0 && !s.have_env && s.n_samples <= sample_max && !deep &&
                           (tex ? tex_off == nullptr : s.ext_flags == 0 || vol_wf);
    r.tex = tex;
    r.maps = tex && s.have_maps;
    if (wavefront) {
        r.family = kRouteWavefront;
        r.vol = vol_wf;
        r.vine = s.n_vine > 0 && !vol_wf;
        r.form = r.maps ? kWfTexMaps : tex ? kWfTex : vol_wf ? kWfVolume : r.vine ? kWfListScan : kWfTree;
        r.kernel = kWgwfNames[r.form][adaptive];
        return r;
    }
    r.ext = s.n_spheres > 0 || s.ext_flags != 0 || tex || s.have_env;
    r.family = s.variant == 2 || r.ext ? kRoutePersistent : s.variant;
    if (s.variant == 2) {  // not silently: the reason and a count are in the stats
        r.fallback = (r.ext && !vol_wf ? kRouteFallbackExtensions : 0) | (deep ? kRouteFallbackDepth : 0) | (s.n_samples > sample_max ? kRouteFallbackSamples : 0);
        r.fallback_counts = true;
    }
    if (r.family == kRouteTile) { r.kernel = "pt_render_kernel"; return r; }
    r.vol = volume;
    r.env = s.have_env;
    r.cut = tex && s.have_cut;
    r.emit = tex && s.have_emit;  // (no call binds both; emission maps would win)
    r.form = r.emit  ? (r.env ? (r.maps ? kFormEnvTexMapsEmit : kFormEnvTexEmit) : (r.maps ? kFormTexMapsEmit : kFormTexEmit))
             : r.cut ? (r.env ? (r.maps ? kFormEnvTexMapsCut : kFormEnvTexCut) : (r.maps ? kFormTexMapsCut : kFormTexCut))
             : r.env ? (r.maps ? kFormEnvTexMaps : tex ? kFormEnvTex : kFormEnv)
             : tex   ? (r.vol ? (r.maps ? kFormTexVolMaps : kFormTexVol) : (r.maps ? kFormTexMaps : kFormTex))
             : r.vol ? kFormVol : r.ext ? kFormExt : kFormPlain;
    r.kernel = kPersistentNames[r.form];
    return r;
}

}  // namespace glrt_detail
