"""ctypes binding of libglrtx.so (include/glrtx.h) -- the HIP device layer.

There is no CPU fallback: if the library is missing or no gfx950 device is
present, construction raises.  Tests and bench call the device path only
through this C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .host import LIB_DIR, PKG_ROOT, EnvCfg, ENV_ESCAPE, ENV_SAMPLED  # noqa: F401  (device.EnvCfg is glrtx_env_cfg)

GLRTX_OK = 0
GLRTX_EINVAL, GLRTX_EDEVICE, GLRTX_ESCENE, GLRTX_EDEPTH, GLRTX_ENOMEM, GLRTX_EBUSY = -1, -2, -3, -4, -5, -6
EXT_DIELECTRIC, EXT_WHITTED = 1, 2
EXT_VOLUME = 4  # the reference's volume branch (ENABLE_VOLUME, raytrace.frag:4); pinned, see upload_volume
VMATH_LOG, VMATH_EXP, VMATH_ACOS, VMATH_BLACKBODY = 0, 1, 2, 3
FALLBACK_DEPTH, FALLBACK_SAMPLES, FALLBACK_EXTENSIONS = 1, 2, 4


class Params(C.Structure):
    _fields_ = [("c2w", C.c_float * 16), ("s2c", C.c_float * 16), ("aperture", C.c_float), ("focal", C.c_float),
                ("seed", C.c_float * 2), ("n_samples", C.c_int32), ("max_depth", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("rays_untraced", C.c_uint64), ("paths", C.c_uint64), ("launches", C.c_uint64), ("kernel_launches", C.c_uint64),
                ("kernel_ms_total", C.c_double), ("accumulate_ms_total", C.c_double), ("kernel_ms_last", C.c_float),
                ("frames_last", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("owned_rows", C.c_int32),
                ("stack_entries", C.c_int32), ("lds_bytes", C.c_int32), ("n_tri", C.c_int32), ("n_fork", C.c_int32),
                ("n_mat", C.c_int32), ("n_light", C.c_int32), ("variant_last", C.c_int32), ("fallback_last", C.c_int32),
                ("resolve_ms_last", C.c_float), ("node_fetch_last", C.c_int32), ("fallback_launches", C.c_uint64),
                ("pipe_slots", C.c_int32), ("pipe_resident_max", C.c_int32), ("device_error_pending", C.c_int32), ("wf_state_mib", C.c_int32),
                ("shadow_limited", C.c_int32), ("node_layout_last", C.c_int32), ("feed_launches", C.c_uint64), ("feed_appended", C.c_uint64)]


class Adaptive(C.Structure):
    """glrtx_adaptive: a tile retires once its error E <= threshold (threshold < 0: nothing retires) and every pixel has min_samples (>= 2) samples."""
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_int32)]


class DenoiseCfg(C.Structure):
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("demodulate", C.c_int)]


class DenoiseVarCfg(C.Structure):
    """glrtx_denoise_var_cfg (device.denoise_var_cfg fills in glrt_amd.host.DENOISE_VAR_DEFAULTS)."""
    _fields_ = [("iterations", C.c_int), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("demodulate", C.c_int)]


class ReprojectCfg(C.Structure):
    """glrtx_reproject_cfg; ReprojectCfg.default() holds glrt_amd.host.REPROJECT_DEFAULTS."""
    _fields_ = [("max_history", C.c_int), ("depth_tolerance", C.c_float), ("normal_tolerance", C.c_float)]

    @classmethod
    def default(cls, max_history=None, depth_tolerance=None, normal_tolerance=None):
        from .host import REPROJECT_DEFAULTS as d
        pick = lambda v, k: d[k] if v is None else v
        return cls(int(pick(max_history, "max_history")), float(pick(depth_tolerance, "depth_tolerance")), float(pick(normal_tolerance, "normal_tolerance")))


class TonemapCfg(C.Structure):
    """glrtx_tonemap_cfg (include/glrtx.h "Tone mapping"); TonemapCfg.default(**fields) holds glrt_amd.host.TONEMAP_DEFAULTS.  op: 0 clamp, 1 Reinhard, 2 ACES
    (or one of TONEMAP_OPS' names)."""
    _fields_ = [("op", C.c_int), ("source", C.c_int), ("auto_exposure", C.c_int), ("exposure", C.c_float), ("key", C.c_float), ("low_permille", C.c_int),
                ("high_permille", C.c_int), ("adapt", C.c_float), ("white", C.c_float), ("gamma", C.c_float), ("flip_y", C.c_int)]

    @classmethod
    def default(cls, **fields):
        from .host import TONEMAP_DEFAULTS, TONEMAP_OPS
        d = dict(TONEMAP_DEFAULTS)
        unknown = set(fields) - set(d)
        if unknown:
            raise TypeError(f"TonemapCfg: unknown field(s) {sorted(unknown)}")
        d.update({k: v for k, v in fields.items() if v is not None})
        if isinstance(d["op"], str):
            d["op"] = TONEMAP_OPS[d["op"]]
        c = cls()
        for name, ctype in cls._fields_:
            setattr(c, name, float(d[name]) if ctype is C.c_float else int(d[name]))
        return c


class Exposure(C.Structure):
    """glrtx_exposure: the last measurement's histogram, N, K, mean_log2, target, E, and the number of measurements since create / reset."""
    _fields_ = [("hist", C.c_uint32 * 256), ("counted", C.c_uint64), ("kept", C.c_uint64), ("mean_log2", C.c_float), ("target", C.c_float),
                ("exposure", C.c_float), ("measurements", C.c_int)]


def _tonemap_cfg(cfg, fields) -> TonemapCfg:
    if cfg is not None and fields:
        raise TypeError("give a TonemapCfg or its fields, not both")
    return cfg if cfg is not None else TonemapCfg.default(**fields)


class BloomCfg(C.Structure):
    """glrtx_bloom_cfg (include/glrtx.h "Bloom"); BloomCfg.default(**fields) holds glrt_amd.host.BLOOM_DEFAULTS."""
    _fields_ = [("source", C.c_int), ("threshold", C.c_float), ("strength", C.c_float), ("levels", C.c_int)]

    @classmethod
    def default(cls, **fields):
        from .host import BLOOM_DEFAULTS
        d = dict(BLOOM_DEFAULTS)
        unknown = set(fields) - set(d)
        if unknown:
            raise TypeError(f"BloomCfg: unknown field(s) {sorted(unknown)}")
        d.update({k: v for k, v in fields.items() if v is not None})
        c = cls()
        for name, ctype in cls._fields_:
            setattr(c, name, float(d[name]) if ctype is C.c_float else int(d[name]))
        return c


def _bloom_cfg(cfg, fields) -> BloomCfg:
    if cfg is not None and fields:
        raise TypeError("give a BloomCfg or its fields, not both")
    return cfg if cfg is not None else BloomCfg.default(**fields)


class ReweightCfg(C.Structure):
    """glrtx_reweight_cfg (include/glrtx.h "Firefly re-weighting"); reweight_cfg() holds glrt_amd.host.REWEIGHT_DEFAULTS."""
    _fields_ = [("kappa", C.c_float)]


def reweight_cfg(kappa=None) -> ReweightCfg:
    from .host import REWEIGHT_DEFAULTS
    return ReweightCfg(float(REWEIGHT_DEFAULTS["kappa"] if kappa is None else kappa))


class Image(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("pitch_bytes", C.c_size_t), ("width", C.c_int32), ("rows", C.c_int32), ("frame", C.c_uint64)]


class PresentStats(C.Structure):
    _fields_ = [("images", C.c_uint64), ("delivered", C.c_uint64), ("dropped", C.c_uint64), ("busy_returns", C.c_uint64),
                ("ring_images", C.c_int32), ("pending", C.c_int32), ("held", C.c_int32), ("copies_last", C.c_int32),
                ("pass_ms_last", C.c_float), ("reserved", C.c_int32)]


class Presented:
    """An acquired image (glrtx_present_acquire): `frame`, and `rgba`, a (rows, width, 4) uint8 view of the pinned ring image -- zero-copy, valid until released."""

    def __init__(self, img: Image):
        self.img = img
        self.frame = int(img.frame)
        n = int(img.rows) * int(img.pitch_bytes)
        buf = (C.c_uint8 * max(n, 1)).from_address(img.rgba) if img.rgba else (C.c_uint8 * 1)()
        self.rgba = np.ctypeslib.as_array(buf)[:n].reshape(int(img.rows), int(img.width), 4)


EXPORTS = ["glrtx_abi_version", "glrtx_create", "glrtx_destroy", "glrtx_last_error", "glrtx_upload_scene", "glrtx_build_lbvh", "glrtx_build_bvh_sah",
           "glrtx_resize", "glrtx_clear", "glrtx_set_partition", "glrtx_local_row_to_y", "glrtx_bind_accum",
           "glrtx_set_stream", "glrtx_set_variant", "glrtx_set_shadow_range_limit", "glrtx_count_rays", "glrtx_render", "glrtx_render_frames", "glrtx_sync", "glrtx_read_accum",
           "glrtx_accum_device_ptr", "glrtx_resolve_rgba8", "glrtx_get_stats", "glrtx_reset_stats",
           "glrtx_timer_begin", "glrtx_timer_end", "glrtx_upload_spheres", "glrtx_set_extensions",
           "glrtx_group_create", "glrtx_group_destroy", "glrtx_group_last_error", "glrtx_group_size", "glrtx_group_ctx",
           "glrtx_group_upload_scene", "glrtx_group_resize", "glrtx_group_clear", "glrtx_group_render", "glrtx_group_render_frames",
           "glrtx_debug_resolve_burst", "glrtx_hit_histogram", "glrtx_group_sync", "glrtx_group_read_accum", "glrtx_group_resolve_rgba8", "glrtx_group_get_stats", "glrtx_group_gather_copies",
           "glrtx_present_enable", "glrtx_present_acquire", "glrtx_present_release", "glrtx_present_get_stats",
           "glrtx_group_present_enable", "glrtx_group_present_acquire", "glrtx_group_present_release", "glrtx_group_present_get_stats",
           "glrtx_upload_volume", "glrtx_group_upload_volume", "glrtx_debug_volume_math", "glrtx_debug_volume_lookup",
           "glrtx_render_adaptive", "glrtx_adaptive_active_tiles", "glrtx_read_tile_mask", "glrtx_read_adaptive_half", "glrtx_debug_adaptive_select",
           "glrtx_group_render_adaptive", "glrtx_group_adaptive_active_tiles", "glrtx_debug_pack_compact", "glrtx_set_volume_wavefront", "glrtx_set_texture_wavefront",
           "glrtx_render_features", "glrtx_read_features", "glrtx_denoise", "glrtx_read_denoised", "glrtx_resolve_denoised_rgba8", "glrtx_debug_denoise",
           "glrtx_update_vertices", "glrtx_update_vertices_device", "glrtx_group_update_vertices", "glrtx_debug_read_scene",
           "glrtx_trace_rays", "glrtx_trace_rays_device", "glrtx_reproject", "glrtx_reproject_last", "glrtx_debug_reproject",
           "glrtx_track_motion", "glrtx_read_features_geom", "glrtx_reproject_motion", "glrtx_debug_reproject_motion",
           "glrtx_track_moments", "glrtx_render_moments", "glrtx_read_moments", "glrtx_denoise_variance", "glrtx_debug_denoise_variance",
           "glrtx_debug_reproject_moments", "glrtx_debug_reproject_motion_moments", "glrtx_render_adaptive_moments", "glrtx_debug_adaptive_select_moments",
           "glrtx_exposure_measure", "glrtx_exposure_reset", "glrtx_read_exposure", "glrtx_tonemap", "glrtx_read_tonemapped", "glrtx_resolve_tonemapped_rgba8",
           "glrtx_debug_tonemap", "glrtx_debug_tonemap_burst",
           "glrtx_bloom", "glrtx_read_bloomed", "glrtx_tonemap_bloomed", "glrtx_resolve_bloomed_rgba8", "glrtx_debug_bloom", "glrtx_debug_bloom_burst",
           "glrtx_track_cascades", "glrtx_render_cascades", "glrtx_read_cascades", "glrtx_reweight", "glrtx_debug_fold_cascades", "glrtx_debug_reweight",
           "glrtx_debug_reweight_burst", "glrtx_upload_rig", "glrtx_pose", "glrtx_debug_skin", "glrtx_debug_skin_burst",
           "glrtx_upload_morph_targets", "glrtx_pose_morph", "glrtx_pose_dualquat", "glrtx_debug_deform", "glrtx_debug_deform_burst",
           "glrtx_upload_morph_targets_sparse", "glrtx_debug_deform_sparse",
           "glrtx_upload_normal_topology", "glrtx_update_positions", "glrtx_update_positions_device", "glrtx_set_pose_normals",
           "glrtx_debug_rebuild_normals", "glrtx_debug_normals_burst", "glrtx_upload_textures", "glrtx_debug_texture_lookup",
           "glrtx_upload_environment", "glrtx_set_environment_cfg", "glrtx_debug_env_weights", "glrtx_debug_env_sample", "glrtx_debug_env_eval",
           "glrtx_bind_material_maps", "glrtx_debug_map_normal", "glrtx_bind_cutouts", "glrtx_debug_texture_channel", "glrtx_debug_last_kernel",
           "glrtx_bind_emission_maps", "glrtx_debug_light_emission"]

SCENE_BUFFERS = ("nodes", "cnodes", "nrms", "lights", "vine", "root")  # glrtx_debug_read_scene's `which`, in order (GLRTX_SCENE_*)

_lib = None


def lib_path():
    return LIB_DIR / "libglrtx.so"


def lib():
    global _lib
    if _lib is None:
        path = lib_path()
        if not path.exists():
            raise RuntimeError(f"{path} is missing: the HIP extension is not built "
                               f"(run `make -C {PKG_ROOT}` or __graft_entry__.build()); there is no fallback path")
        L = C.CDLL(str(path))
        vp, fp = C.c_void_p, C.POINTER(C.c_float)
        L.glrtx_abi_version.restype = C.c_int
        L.glrtx_create.argtypes = [C.POINTER(vp), C.c_int]
        L.glrtx_destroy.argtypes = [vp]
        L.glrtx_destroy.restype = None
        L.glrtx_last_error.argtypes = [vp]
        L.glrtx_last_error.restype = C.c_char_p
        L.glrtx_upload_scene.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp,
                                         C.c_size_t]
        L.glrtx_build_lbvh.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, fp, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.glrtx_build_bvh_sah.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, fp, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.glrtx_resize.argtypes = [vp, C.c_int, C.c_int]
        L.glrtx_clear.argtypes = [vp]
        L.glrtx_set_partition.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.glrtx_local_row_to_y.argtypes = [vp, C.c_int]
        L.glrtx_bind_accum.argtypes = [vp, vp, C.c_size_t, C.c_int]
        L.glrtx_set_stream.argtypes = [vp, vp]
        L.glrtx_set_variant.argtypes = [vp, C.c_int]
        L.glrtx_set_shadow_range_limit.argtypes = [vp, C.c_int]
        L.glrtx_count_rays.argtypes = [vp, C.c_int]
        L.glrtx_render.argtypes = [vp, C.POINTER(Params)]
        L.glrtx_render_frames.argtypes = [vp, C.POINTER(Params), fp, C.c_int]
        L.glrtx_sync.argtypes = [vp]
        L.glrtx_read_accum.argtypes = [vp, vp, C.c_size_t]
        L.glrtx_accum_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.glrtx_resolve_rgba8.argtypes = [vp, vp, C.c_size_t, C.c_float, C.c_int]
        L.glrtx_get_stats.argtypes = [vp, C.POINTER(Stats)]
        try:  # (ABI 10; tools/gpu_abx.py also loads libraries of earlier rounds for A/B runs)
            L.glrtx_debug_resolve_burst.argtypes = [vp, C.c_float, C.c_int, C.POINTER(C.c_float)]
            L.glrtx_hit_histogram.argtypes = [vp, C.POINTER(Params), C.POINTER(C.c_uint32), C.c_size_t]
        except AttributeError:
            pass
        L.glrtx_reset_stats.argtypes = [vp]
        L.glrtx_timer_begin.argtypes = [vp]
        L.glrtx_timer_end.argtypes = [vp, C.POINTER(C.c_float)]
        L.glrtx_upload_spheres.argtypes = [vp, fp, C.c_size_t]
        L.glrtx_set_extensions.argtypes = [vp, C.c_int]
        L.glrtx_upload_volume.argtypes = [vp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, C.c_float]
        L.glrtx_group_upload_volume.argtypes = [vp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, C.c_float]
        L.glrtx_debug_volume_math.argtypes = [C.c_int, fp, C.c_size_t, fp]
        L.glrtx_debug_volume_lookup.argtypes = [fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_size_t, fp]
        L.glrtx_group_create.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
        L.glrtx_group_destroy.argtypes = [vp]
        L.glrtx_group_destroy.restype = None
        L.glrtx_group_last_error.argtypes = [vp]
        L.glrtx_group_last_error.restype = C.c_char_p
        L.glrtx_group_size.argtypes = [vp]
        L.glrtx_group_ctx.argtypes = [vp, C.c_int]
        L.glrtx_group_ctx.restype = vp
        L.glrtx_group_upload_scene.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t]
        L.glrtx_group_resize.argtypes = [vp, C.c_int, C.c_int]
        L.glrtx_group_clear.argtypes = [vp]
        L.glrtx_group_render.argtypes = [vp, C.POINTER(Params)]
        L.glrtx_group_render_frames.argtypes = [vp, C.POINTER(Params), fp, C.c_int]
        L.glrtx_group_sync.argtypes = [vp]
        L.glrtx_group_read_accum.argtypes = [vp, vp, C.c_size_t]
        L.glrtx_group_resolve_rgba8.argtypes = [vp, vp, C.c_size_t, C.c_float, C.c_int]
        L.glrtx_group_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.glrtx_group_gather_copies.argtypes = [vp]
        L.glrtx_present_enable.argtypes = [vp, C.c_int, C.c_float, C.c_int]
        L.glrtx_present_acquire.argtypes = [vp, C.c_int, C.POINTER(Image)]
        L.glrtx_present_release.argtypes = [vp, C.POINTER(Image)]
        L.glrtx_present_get_stats.argtypes = [vp, C.POINTER(PresentStats)]
        L.glrtx_group_present_enable.argtypes = [vp, C.c_int, C.c_float, C.c_int]
        L.glrtx_group_present_acquire.argtypes = [vp, C.c_int, C.POINTER(Image)]
        L.glrtx_group_present_release.argtypes = [vp, C.POINTER(Image)]
        L.glrtx_group_present_get_stats.argtypes = [vp, C.POINTER(PresentStats)]
        ip, u8p = C.POINTER(C.c_int), C.POINTER(C.c_uint8)
        L.glrtx_render_adaptive.argtypes = [vp, C.POINTER(Params), fp, C.c_int, C.POINTER(Adaptive)]
        L.glrtx_adaptive_active_tiles.argtypes = [vp, ip, ip]
        L.glrtx_read_tile_mask.argtypes = [vp, u8p]
        L.glrtx_read_adaptive_half.argtypes = [vp, vp, C.c_size_t]
        L.glrtx_debug_adaptive_select.argtypes = [fp, fp, C.c_int, C.c_int, C.c_float, C.c_int, u8p, fp, ip, ip]
        L.glrtx_group_render_adaptive.argtypes = [vp, C.POINTER(Params), fp, C.c_int, C.POINTER(Adaptive)]
        L.glrtx_group_adaptive_active_tiles.argtypes = [vp, ip, ip]
        u32p = C.POINTER(C.c_uint32)
        L.glrtx_debug_pack_compact.argtypes = [fp, C.c_size_t] * 5 + [fp, C.c_size_t, ip, u32p, C.c_size_t, fp, C.c_size_t, ip]
        L.glrtx_update_vertices.argtypes = [vp, fp, C.c_size_t]
        L.glrtx_update_vertices_device.argtypes = [vp, vp, C.c_size_t]
        L.glrtx_group_update_vertices.argtypes = [vp, fp, C.c_size_t]
        L.glrtx_trace_rays.argtypes = [vp, fp, C.c_size_t, fp, C.c_int]
        L.glrtx_trace_rays_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_int]
        L.glrtx_debug_read_scene.argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        try:  # (additive to ABI 10: libraries of earlier rounds, which tools/gpu_abx.py loads, lack it)
            L.glrtx_set_volume_wavefront.argtypes = [vp, C.c_int]
            L.glrtx_set_texture_wavefront.argtypes = [vp, C.c_int]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: the denoiser)
            L.glrtx_render_features.argtypes = [vp, C.POINTER(Params)]
            L.glrtx_read_features.argtypes = [vp, vp, vp, C.c_size_t]
            L.glrtx_denoise.argtypes = [vp, C.POINTER(DenoiseCfg)]
            L.glrtx_read_denoised.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_resolve_denoised_rgba8.argtypes = [vp, vp, C.c_size_t, C.c_float, C.c_int]
            L.glrtx_debug_denoise.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.POINTER(DenoiseCfg), fp]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: the reprojection)
            L.glrtx_reproject.argtypes = [vp, C.POINTER(Params), C.POINTER(ReprojectCfg)]
            L.glrtx_reproject_last.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.glrtx_debug_reproject.argtypes = [fp] * 9 + [C.c_int, C.c_int, C.POINTER(ReprojectCfg), fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: reprojection across a geometry move)
            L.glrtx_track_motion.argtypes = [vp, C.c_int]
            L.glrtx_read_features_geom.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_reproject_motion.argtypes = [vp, C.POINTER(Params), C.POINTER(ReprojectCfg)]
            L.glrtx_debug_reproject_motion.argtypes = [fp] * 6 + [C.c_size_t, fp, C.c_size_t, fp, fp, C.c_int, C.c_int, C.POINTER(ReprojectCfg), fp,
                                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: variance guidance)
            L.glrtx_track_moments.argtypes = [vp, C.c_int]
            L.glrtx_render_moments.argtypes = [vp, C.POINTER(Params), fp, C.c_int]
            L.glrtx_read_moments.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_denoise_variance.argtypes = [vp, C.POINTER(DenoiseVarCfg)]
            L.glrtx_debug_denoise_variance.argtypes = [fp, fp, fp, fp, C.c_int, C.c_int, C.POINTER(DenoiseVarCfg), fp, fp]
            L.glrtx_debug_reproject_moments.argtypes = [fp] * 10 + [C.c_int, C.c_int, C.POINTER(ReprojectCfg), fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.glrtx_debug_reproject_motion_moments.argtypes = [fp] * 7 + [C.c_size_t, fp, C.c_size_t, fp, fp, C.c_int, C.c_int, C.POINTER(ReprojectCfg), fp, fp,
                                                               C.POINTER(C.c_int), C.POINTER(C.c_int)]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: the adaptive selection from M)
            L.glrtx_render_adaptive_moments.argtypes = [vp, C.POINTER(Params), fp, C.c_int, C.POINTER(Adaptive)]
            L.glrtx_debug_adaptive_select_moments.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_int, u8p, fp, ip, ip]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: tone mapping)
            tc = C.POINTER(TonemapCfg)
            L.glrtx_exposure_measure.argtypes = [vp, tc]
            L.glrtx_exposure_reset.argtypes = [vp]
            L.glrtx_read_exposure.argtypes = [vp, C.POINTER(Exposure)]
            L.glrtx_tonemap.argtypes = [vp, tc]
            L.glrtx_read_tonemapped.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_resolve_tonemapped_rgba8.argtypes = [vp, vp, C.c_size_t, tc]
            L.glrtx_debug_tonemap.argtypes = [fp, C.c_int, C.c_int, tc, fp, C.POINTER(Exposure), fp, C.POINTER(C.c_uint8)]
            L.glrtx_debug_tonemap_burst.argtypes = [vp, tc, C.c_int, C.c_int, C.POINTER(C.c_float)]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: bloom)
            tc, bc = C.POINTER(TonemapCfg), C.POINTER(BloomCfg)
            L.glrtx_bloom.argtypes = [vp, bc]
            L.glrtx_read_bloomed.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_tonemap_bloomed.argtypes = [vp, tc]
            L.glrtx_resolve_bloomed_rgba8.argtypes = [vp, vp, C.c_size_t, tc]
            L.glrtx_debug_bloom.argtypes = [fp, C.c_int, C.c_int, bc, fp, fp]
            L.glrtx_debug_bloom_burst.argtypes = [vp, bc, C.c_int, C.POINTER(C.c_float)]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: firefly re-weighting)
            rc = C.POINTER(ReweightCfg)
            L.glrtx_track_cascades.argtypes = [vp, C.c_int, C.c_float]
            L.glrtx_render_cascades.argtypes = [vp, C.POINTER(Params), fp, C.c_int]
            L.glrtx_read_cascades.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_reweight.argtypes = [vp, rc]
            L.glrtx_debug_fold_cascades.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, fp, fp]
            L.glrtx_debug_reweight.argtypes = [fp, C.c_int, C.c_int, rc, fp]
            L.glrtx_debug_reweight_burst.argtypes = [vp, rc, C.c_int, C.POINTER(C.c_float)]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: posing)
            i32p = C.POINTER(C.c_int32)
            L.glrtx_upload_rig.argtypes = [vp, fp, C.c_size_t, i32p, fp, C.c_int]
            L.glrtx_pose.argtypes = [vp, fp, C.c_int]
            L.glrtx_debug_skin.argtypes = [fp, C.c_size_t, i32p, fp, fp, C.c_int, fp]
            L.glrtx_debug_skin_burst.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
            L.glrtx_upload_morph_targets.argtypes = [vp, fp, C.c_int, C.c_size_t]
            L.glrtx_pose_morph.argtypes = [vp, fp, C.c_int, fp, C.c_int]
            L.glrtx_pose_dualquat.argtypes = [vp, fp, C.c_int, fp, C.c_int]
            L.glrtx_debug_deform.argtypes = [fp, C.c_size_t, i32p, fp, fp, C.c_int, C.c_int, fp, fp, C.c_int, fp]
            L.glrtx_debug_deform_burst.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
            u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
            L.glrtx_upload_morph_targets_sparse.argtypes = [vp, u64p, u32p, fp, C.c_int, C.c_size_t]
            L.glrtx_debug_deform_sparse.argtypes = [fp, C.c_size_t, i32p, fp, fp, C.c_int, C.c_int, u64p, u32p, fp, fp, C.c_int, fp]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: rebuilding normals)
            u8p = C.POINTER(C.c_uint8)
            L.glrtx_upload_normal_topology.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, C.c_uint]
            L.glrtx_update_positions.argtypes = [vp, fp, C.c_size_t]
            L.glrtx_update_positions_device.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_set_pose_normals.argtypes = [vp, C.c_int]
            L.glrtx_debug_rebuild_normals.argtypes = [fp, C.c_size_t, fp, C.c_size_t, C.POINTER(C.c_uint32), u8p, fp]
            L.glrtx_debug_normals_burst.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: textures)
            i32p = C.POINTER(C.c_int32)
            L.glrtx_upload_textures.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32p, C.c_size_t]
            L.glrtx_debug_texture_lookup.argtypes = [vp, C.c_size_t, vp, C.c_size_t, i32p, fp, C.c_size_t, fp]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: the environment)
            L.glrtx_upload_environment.argtypes = [vp, vp, vp, C.c_size_t, vp]
            L.glrtx_set_environment_cfg.argtypes = [vp, vp]
            L.glrtx_debug_env_weights.argtypes = [vp, vp, C.c_size_t, vp, fp, C.POINTER(C.c_int32)]
            L.glrtx_debug_env_sample.argtypes = [vp, vp, C.c_size_t, vp, fp, C.c_size_t, fp]
            L.glrtx_debug_env_eval.argtypes = [vp, vp, C.c_size_t, vp, fp, C.c_size_t, fp]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: material maps)
            L.glrtx_bind_material_maps.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_debug_map_normal.argtypes = [fp, C.c_size_t, C.c_float, fp]
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: cutouts)
            i32p = C.POINTER(C.c_int32)
            L.glrtx_bind_cutouts.argtypes = [vp, vp, C.c_size_t]
            L.glrtx_debug_texture_channel.argtypes = [vp, C.c_size_t, vp, C.c_size_t, i32p, i32p, fp, C.c_size_t, fp]
            L.glrtx_debug_last_kernel.argtypes = [vp]
            L.glrtx_debug_last_kernel.restype = C.c_char_p
        except AttributeError:
            pass
        try:  # (additive to ABI 10 as well: emission maps)
            i32p = C.POINTER(C.c_int32)
            L.glrtx_bind_emission_maps.argtypes = [vp, i32p, C.c_size_t]
            L.glrtx_debug_light_emission.argtypes = [vp, i32p, fp, C.c_size_t, fp]
        except AttributeError:
            pass
        _lib = L
    return _lib


class GlrtxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"glrtx error {code}: {msg}")
        self.code = code


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def make_params(p) -> Params:
    r = Params()
    r.c2w[:] = list(_f32(p["c2w"]).reshape(16))
    r.s2c[:] = list(_f32(p["s2c"]).reshape(16))
    r.aperture = p.get("aperture", 0.0)
    r.focal = p.get("focal", 1.0)
    r.seed[:] = [p["seed"][0], p["seed"][1]]
    r.n_samples = int(p["n_samples"])
    r.max_depth = int(p["max_depth"])
    return r


def _upload_volume(fn, h, density, temperature, bbox_min, bbox_max, density_max):
    lo, hi = _f32(np.asarray(bbox_min).reshape(3)), _f32(np.asarray(bbox_max).reshape(3))
    if density is None:
        return fn(h, None, None, 0, 0, 0, _fp(lo), _fp(hi), 0.0)
    d, t = _f32(density), _f32(temperature)
    if d.ndim != 3 or t.shape != d.shape:
        raise ValueError(f"upload_volume: grids must be (nz, ny, nx) and of one shape, got {d.shape} and {t.shape}")
    nz, ny, nx = d.shape
    dm = float(d.max()) if density_max is None else float(density_max)
    return fn(h, _fp(d), _fp(t), nx, ny, nz, _fp(lo), _fp(hi), dm)


def volume_math(op, x):
    """glrtx_debug_volume_math on the current device: the kernel's log / exp / acos / blackBody (VMATH_*) of float32 array x."""
    L = lib()
    a = _f32(np.asarray(x).reshape(-1))
    out = np.zeros((a.size, 3) if op == VMATH_BLACKBODY else a.size, np.float32)
    rc = L.glrtx_debug_volume_math(int(op), _fp(a), a.size, _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def volume_lookup(grid, bbox_min, bbox_max, pos):
    """glrtx_debug_volume_lookup on the current device: the kernel's trilinear lookup of grid (nz, ny, nx) at pos (n, 3)."""
    L = lib()
    g = _f32(grid)
    p = _f32(np.asarray(pos).reshape(-1, 3))
    lo, hi = _f32(np.asarray(bbox_min).reshape(3)), _f32(np.asarray(bbox_max).reshape(3))
    out = np.zeros(p.shape[0], np.float32)
    nz, ny, nx = g.shape
    rc = L.glrtx_debug_volume_lookup(_fp(g), nx, ny, nz, _fp(lo), _fp(hi), _fp(p), p.shape[0], _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def debug_texture_lookup(textures, which, st):
    """glrtx_debug_texture_lookup on the current device: the kernels' tex_lookup (include/glrtx.h "Textures").  Arguments and result as host.texture_lookup's."""
    from .host import pack_textures
    L = lib()
    desc, blob = pack_textures(textures)
    w = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
    c = _f32(st).reshape(-1, 2)
    if c.shape[0] != w.size:
        raise ValueError(f"debug_texture_lookup: {w.size} texture indices, {c.shape[0]} coordinates")
    out = np.zeros((w.size, 3), np.float32)
    rc = L.glrtx_debug_texture_lookup(desc.ctypes.data, desc.size, blob.ctypes.data, blob.size, w.ctypes.data_as(C.POINTER(C.c_int32)), _fp(c), w.size, _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def debug_texture_channel(textures, which, channel, st):
    """glrtx_debug_texture_channel on the current device: the kernels' tex_lookup_channel (include/glrtx.h "Cutouts").  Arguments and result as
    host.texture_channel's."""
    from .host import pack_textures
    L = lib()
    desc, blob = pack_textures(textures)
    w = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
    ch = np.ascontiguousarray(np.broadcast_to(np.asarray(channel, np.int32), w.shape))
    c = _f32(st).reshape(-1, 2)
    if c.shape[0] != w.size:
        raise ValueError(f"debug_texture_channel: {w.size} texture indices, {c.shape[0]} coordinates")
    out = np.zeros(w.size, np.float32)
    i32p = C.POINTER(C.c_int32)
    rc = L.glrtx_debug_texture_channel(desc.ctypes.data, desc.size, blob.ctypes.data, blob.size, w.ctypes.data_as(i32p), ch.ctypes.data_as(i32p), _fp(c), w.size,
                                       _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def debug_light_emission(dev, lid, u):
    """glrtx_debug_light_emission on dev (a Device with emission maps bound): the kernels' sampled-side statement (include/glrtx.h "Emission maps") on the
    context's own scene, set and bindings.  lid (n,) light indices, u (n, 2) raw uniforms; returns (n, 5) float32 {s, t, Le.rgb}, as host.light_emission."""
    return dev.debug_light_emission(lid, u)


def debug_map_normal(records, scale=1.0):
    """glrtx_debug_map_normal on the current device: the kernels' map_normal (include/glrtx.h "Material maps").  Arguments and result as host.map_normal's."""
    from .host import MAP_RECORD_FLOATS
    L = lib()
    r = np.ascontiguousarray(records, np.float32).reshape(-1, MAP_RECORD_FLOATS)
    out = np.zeros((r.shape[0], 3), np.float32)
    rc = L.glrtx_debug_map_normal(_fp(r), r.shape[0], C.c_float(scale), _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def _debug_env(name, env_map, cfg, *rest):
    from .host import pack_environment
    L = lib()
    desc, blob = pack_environment(env_map)
    rc = getattr(L, name)(desc.ctypes.data, blob.ctypes.data, blob.size, C.addressof(cfg) if cfg is not None else None, *rest)
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())


def debug_env_weights(env_map, cfg):
    """glrtx_debug_env_weights on the current device: env_weights_kernel (include/glrtx.h "Environment").  Arguments and result as host.env_weights's."""
    from .host import pack_environment
    desc, _ = pack_environment(env_map)
    g = int(cfg.grid) if cfg is not None and 0 < int(cfg.grid) <= 1024 else min(int(desc["width"][0]), 256)
    out, grid = np.zeros(max(g, 1) ** 2, np.float32), C.c_int32(0)
    _debug_env("glrtx_debug_env_weights", env_map, cfg, _fp(out), C.byref(grid))
    return out.reshape(grid.value, grid.value)


def debug_env_sample(env_map, cfg, u):
    """glrtx_debug_env_sample on the current device: the kernels' env_sample.  Arguments and result as host.env_sample's."""
    q = _f32(u).reshape(-1, 6)
    out = np.zeros((q.shape[0], 8), np.float32)
    _debug_env("glrtx_debug_env_sample", env_map, cfg, _fp(q), q.shape[0], _fp(out))
    return out


def debug_env_eval(env_map, cfg, dirs):
    """glrtx_debug_env_eval on the current device: the kernels' env_eval.  Arguments and result as host.env_eval's."""
    d = _f32(dirs).reshape(-1, 3)
    out = np.zeros((d.shape[0], 4), np.float32)
    _debug_env("glrtx_debug_env_eval", env_map, cfg, _fp(d), d.shape[0], _fp(out))
    return out


def adaptive_select(accum, half, threshold, min_samples):
    """glrtx_debug_adaptive_select on the current device: the selection kernels on accum / half (rows, width, 4) float32.
    Returns (mask (tiles_y, tiles_x) uint8, E (tiles_y, tiles_x) float32 -- NaN as 0x7FC00000 --, ascending list of active tiles)."""
    L = lib()
    a, h = _f32(accum), _f32(half)
    if a.ndim != 3 or a.shape[2] != 4 or h.shape != a.shape:
        raise ValueError(f"adaptive_select: accum and half must be (rows, width, 4) of one shape, got {a.shape} and {h.shape}")
    rows, width = a.shape[:2]
    ty, tx = (rows + 7) // 8, (width + 7) // 8
    mask = np.zeros((ty, tx), np.uint8)
    err = np.zeros((ty, tx), np.float32)
    lst = np.zeros(ty * tx, np.int32)
    n = C.c_int(0)
    rc = L.glrtx_debug_adaptive_select(_fp(a), _fp(h), width, rows, float(threshold), int(min_samples), mask.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(err),
                                       lst.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return mask, err, lst[:n.value].copy()


def adaptive_select_moments(moments, threshold, min_samples):
    """glrtx_debug_adaptive_select_moments on the current device: the selection kernels of render_adaptive_moments on a moments plane (rows, width, 4) float32.
    Returns (mask (tiles_y, tiles_x) uint8, E (tiles_y, tiles_x) float32 -- NaN as 0x7FC00000 --, ascending list of active tiles)."""
    L = lib()
    m = _f32(moments)
    if m.ndim != 3 or m.shape[2] != 4:
        raise ValueError(f"adaptive_select_moments: moments must be (rows, width, 4), got {m.shape}")
    rows, width = m.shape[:2]
    ty, tx = (rows + 7) // 8, (width + 7) // 8
    mask = np.zeros((ty, tx), np.uint8)
    err = np.zeros((ty, tx), np.float32)
    lst = np.zeros(ty * tx, np.int32)
    n = C.c_int(0)
    rc = L.glrtx_debug_adaptive_select_moments(_fp(m), width, rows, float(threshold), int(min_samples), mask.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(err),
                                               lst.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return mask, err, lst[:n.value].copy()


def denoise_cfg(iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None) -> DenoiseCfg:
    """A glrtx_denoise_cfg; None takes the default (glrt_amd.host.DENOISE_DEFAULTS)."""
    from .host import DENOISE_DEFAULTS as d
    pick = lambda v, k: d[k] if v is None else v
    return DenoiseCfg(int(pick(iterations, "iterations")), float(pick(sigma_color, "sigma_color")), float(pick(sigma_normal, "sigma_normal")),
                      float(pick(sigma_depth, "sigma_depth")), int(bool(pick(demodulate, "demodulate"))))


def debug_denoise(accum, normal_depth, albedo_id, **cfg):
    """glrtx_debug_denoise on the current device: the filter's kernels on (rows, width, 4) float32 arrays.  Returns D, float4(rgb, 1) per pixel."""
    L = lib()
    a, n, al = _f32(accum), _f32(normal_depth), _f32(albedo_id)
    if a.ndim != 3 or a.shape[2] != 4 or n.shape != a.shape or al.shape != a.shape:
        raise ValueError(f"debug_denoise: three (rows, width, 4) arrays of one shape expected, got {a.shape}, {n.shape}, {al.shape}")
    out = np.zeros_like(a)
    c = denoise_cfg(**cfg)
    rc = L.glrtx_debug_denoise(_fp(a), _fp(n), _fp(al), a.shape[1], a.shape[0], C.byref(c), _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def denoise_var_cfg(iterations=None, sigma_lum=None, sigma_normal=None, sigma_depth=None, demodulate=None) -> DenoiseVarCfg:
    """A glrtx_denoise_var_cfg; None takes the default (glrt_amd.host.DENOISE_VAR_DEFAULTS)."""
    from .host import DENOISE_VAR_DEFAULTS as d
    pick = lambda v, k: d[k] if v is None else v
    return DenoiseVarCfg(int(pick(iterations, "iterations")), float(pick(sigma_lum, "sigma_lum")), float(pick(sigma_normal, "sigma_normal")),
                         float(pick(sigma_depth, "sigma_depth")), int(bool(pick(demodulate, "demodulate"))))


def debug_denoise_variance(accum, moments, normal_depth, albedo_id, return_v0=False, **cfg):
    """glrtx_debug_denoise_variance on the current device: the variance pass and the variance-guided filter on (rows, width, 4) float32 arrays.  Returns D,
    float4(rgb, 1) per pixel; with return_v0 (D, V0), V0 (rows, width) float32."""
    L = lib()
    arr = [_f32(v) for v in (accum, moments, normal_depth, albedo_id)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"debug_denoise_variance: four (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    out = np.zeros_like(a)
    v0 = np.zeros(a.shape[:2], np.float32)
    c = denoise_var_cfg(**cfg)
    rc = L.glrtx_debug_denoise_variance(*[_fp(v) for v in arr], a.shape[1], a.shape[0], C.byref(c), _fp(out), _fp(v0) if return_v0 else None)
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return (out, v0) if return_v0 else out


def debug_tonemap(src, exposure_in=None, cfg=None, **fields):
    """glrtx_debug_tonemap on the current device: one exposure measurement (exposure_in: the previous E, None for a first one), the curve and the fused resolve
    on a (rows, width, 4) float32 array.  Returns (Exposure, T (rows, width, 4) float32, bytes (rows, width, 4) uint8)."""
    L = lib()
    a = _f32(src)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"debug_tonemap: a (rows, width, 4) array expected, got {a.shape}")
    c = _tonemap_cfg(cfg, fields)
    e, t, b = Exposure(), np.zeros_like(a), np.zeros(a.shape, np.uint8)
    prev = None if exposure_in is None else C.c_float(float(exposure_in))
    rc = L.glrtx_debug_tonemap(_fp(a), a.shape[1], a.shape[0], C.byref(c), None if prev is None else C.byref(prev), C.byref(e), _fp(t),
                               b.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return e, t, b


def debug_bloom(src, cfg=None, **fields):
    """glrtx_debug_bloom on the current device: the bloom kernels on a (rows, width, 4) float32 array.  Returns (d, B): d the planes D_1 .. D_levels packed back
    to back, (n, 4) float32 with w = 0, as they stand before the up chain; B (rows, width, 4) float32."""
    from .host import bloom_texels
    L = lib()
    a = _f32(src)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"debug_bloom: a (rows, width, 4) array expected, got {a.shape}")
    c = _bloom_cfg(cfg, fields)
    d, b = np.zeros((bloom_texels(a.shape[1], a.shape[0], min(max(c.levels, 1), 8)), 4), np.float32), np.zeros_like(a)
    rc = L.glrtx_debug_bloom(_fp(a), a.shape[1], a.shape[0], C.byref(c), _fp(d), _fp(b))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return d, b


def debug_fold_cascades(accum, cascades, frames, start=None):
    """glrtx_debug_fold_cascades on the current device: the accumulation pass with the cascade sink on packed arrays -- accum (rows, width, 4), cascades
    (6, rows, width, 4), frames (n, rows, width, 4), one sample each.  Returns (accum_out, cascades_out)."""
    from .host import REWEIGHT_DEFAULTS
    L = lib()
    a, c, f = _f32(accum), _f32(cascades), _f32(frames)
    if a.ndim != 3 or a.shape[2] != 4 or c.shape != (6,) + a.shape or f.ndim != 4 or f.shape[1:] != a.shape:
        raise ValueError(f"debug_fold_cascades: (rows, width, 4), (6, rows, width, 4) and (n, rows, width, 4) expected, got {a.shape}, {c.shape}, {f.shape}")
    ao, co = np.zeros_like(a), np.zeros_like(c)
    rc = L.glrtx_debug_fold_cascades(_fp(a), _fp(c), _fp(f) if f.shape[0] else None, f.shape[0], a.shape[1], a.shape[0],
                                     float(REWEIGHT_DEFAULTS["start"] if start is None else start), _fp(ao), _fp(co))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return ao, co


def debug_reweight(cascades, cfg=None, kappa=None):
    """glrtx_debug_reweight on the current device: the resolve kernel on cascade planes (6, rows, width, 4).  Returns D (rows, width, 4) float32."""
    L = lib()
    c = _f32(cascades)
    if c.ndim != 4 or c.shape[0] != 6 or c.shape[3] != 4:
        raise ValueError(f"debug_reweight: cascades must be (6, rows, width, 4), got {c.shape}")
    k = cfg if cfg is not None else reweight_cfg(kappa)
    out = np.zeros(c.shape[1:], np.float32)
    rc = L.glrtx_debug_reweight(_fp(c), c.shape[2], c.shape[1], C.byref(k), _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def debug_reproject(accum, n0, a0, n1, a1, prev, cur, **cfg):
    """glrtx_debug_reproject on the current device: the reprojection kernel on (rows, width, 4) float32 arrays (the old view's accumulator and planes, the new
    view's planes) and the two cameras (dicts with c2w and s2c).  Returns (out, carried, hit_pixels)."""
    L = lib()
    arr = [_f32(v) for v in (accum, n0, a0, n1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"debug_reproject: five (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    mats = [_f32(np.asarray(m).reshape(16)) for m in (prev["c2w"], prev["s2c"], cur["c2w"], cur["s2c"])]
    out = np.zeros_like(a)
    c = ReprojectCfg.default(**cfg)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = L.glrtx_debug_reproject(*[_fp(v) for v in arr], *[_fp(m) for m in mats], a.shape[1], a.shape[0], C.byref(c), _fp(out), C.byref(carried), C.byref(hits))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out, int(carried.value), int(hits.value)


def debug_reproject_motion(accum, n0, a0, g1, a1, vert_prev, tri, prev, **cfg):
    """glrtx_debug_reproject_motion on the current device: the motion-aware reprojection kernel on (rows, width, 4) float32 arrays (the old view's accumulator
    and planes, the new view's geometry and albedo planes), the vertices as they stood at the old view, the triangles, and the old view's camera (a dict with
    c2w and s2c).  Returns (out, carried, hit_pixels)."""
    L = lib()
    arr = [_f32(v) for v in (accum, n0, a0, g1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"debug_reproject_motion: five (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    vert, tr = _f32(vert_prev).reshape(-1, 15), _f32(tri).reshape(-1, 4)
    mats = [_f32(np.asarray(m).reshape(16)) for m in (prev["c2w"], prev["s2c"])]
    out = np.zeros_like(a)
    c = ReprojectCfg.default(**cfg)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = L.glrtx_debug_reproject_motion(*[_fp(v) for v in arr], _fp(vert), vert.shape[0], _fp(tr), tr.shape[0], *[_fp(m) for m in mats], a.shape[1], a.shape[0],
                                        C.byref(c), _fp(out), C.byref(carried), C.byref(hits))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out, int(carried.value), int(hits.value)


def debug_reproject_moments(accum, moments, n0, a0, n1, a1, prev, cur, **cfg):
    """glrtx_debug_reproject_moments on the current device: debug_reproject with the old view's moments plane M carried through the same taps.  Returns
    (out, moments_out, carried, hit_pixels)."""
    L = lib()
    arr = [_f32(v) for v in (accum, moments, n0, a0, n1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"debug_reproject_moments: six (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    mats = [_f32(np.asarray(m).reshape(16)) for m in (prev["c2w"], prev["s2c"], cur["c2w"], cur["s2c"])]
    out, mo = np.zeros_like(a), np.zeros_like(a)
    c = ReprojectCfg.default(**cfg)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = L.glrtx_debug_reproject_moments(*[_fp(v) for v in arr], *[_fp(m) for m in mats], a.shape[1], a.shape[0], C.byref(c), _fp(out), _fp(mo), C.byref(carried),
                                         C.byref(hits))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out, mo, int(carried.value), int(hits.value)


def debug_reproject_motion_moments(accum, moments, n0, a0, g1, a1, vert_prev, tri, prev, **cfg):
    """glrtx_debug_reproject_motion_moments on the current device: debug_reproject_motion with the old view's moments plane M carried.  Returns
    (out, moments_out, carried, hit_pixels)."""
    L = lib()
    arr = [_f32(v) for v in (accum, moments, n0, a0, g1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"debug_reproject_motion_moments: six (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    vert, tr = _f32(vert_prev).reshape(-1, 15), _f32(tri).reshape(-1, 4)
    mats = [_f32(np.asarray(m).reshape(16)) for m in (prev["c2w"], prev["s2c"])]
    out, mo = np.zeros_like(a), np.zeros_like(a)
    c = ReprojectCfg.default(**cfg)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = L.glrtx_debug_reproject_motion_moments(*[_fp(v) for v in arr], _fp(vert), vert.shape[0], _fp(tr), tr.shape[0], *[_fp(m) for m in mats], a.shape[1],
                                                a.shape[0], C.byref(c), _fp(out), _fp(mo), C.byref(carried), C.byref(hits))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out, mo, int(carried.value), int(hits.value)


def debug_skin(rest, bones, weights, matrices):
    """glrtx_debug_skin on the current device: the skinning kernel alone on a rig's arrays -- rest (n, 15) float32, bones (n, 4) int32, weights (n, 4) float32,
    matrices (n_bones, 12) float32.  Returns the posed vertices (n, 15) float32."""
    from .host import rig_arrays
    L = lib()
    r, b, w, m = rig_arrays("debug_skin", rest, bones, weights, matrices)
    out = np.zeros_like(r)
    rc = L.glrtx_debug_skin(_fp(r), r.shape[0], b.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), _fp(m), m.shape[0], _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def debug_deform(rest, bones, weights, bone_data, mode=0, deltas=None, morph_weights=None):
    """glrtx_debug_deform on the current device: the deform kernel alone -- the rig of debug_skin; bone_data (n_bones, 12) matrices (mode 0) or (n_bones, 8) dual
    quaternions (mode 1); deltas (n_targets, n, 6) float32 and morph_weights (n_targets,) float32, or neither.  Returns the deformed vertices (n, 15) float32."""
    from .host import deform_arrays
    L = lib()
    r, b, w, m, d, mw = deform_arrays("debug_deform", rest, bones, weights, bone_data, mode, deltas, morph_weights)
    out = np.zeros_like(r)
    rc = L.glrtx_debug_deform(_fp(r), r.shape[0], b.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), _fp(m), m.shape[0], int(mode),
                              _fp(d) if mw.size else None, _fp(mw) if mw.size else None, mw.size, _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def debug_deform_sparse(rest, bones, weights, bone_data, mode=0, offsets=None, vertex=None, deltas=None, morph_weights=None):
    """glrtx_debug_deform_sparse on the current device: the sparse deform kernel alone -- the rig and bone data of debug_deform; the set as offsets
    (n_targets + 1,) uint64, vertex (nnz,) uint32, deltas (nnz, 6) float32; morph_weights (n_targets,) float32.  Returns the deformed vertices (n, 15) float32."""
    from .host import deform_arrays, sparse_arrays, sparse_pointers
    L = lib()
    r, b, w, m, _, _ = deform_arrays("debug_deform_sparse", rest, bones, weights, bone_data, mode, None, None)
    o, v, d = sparse_arrays("debug_deform_sparse", offsets, vertex, deltas)
    mw = np.zeros(0, np.float32) if morph_weights is None else _f32(morph_weights).reshape(-1)
    if mw.size != o.size - 1:
        raise ValueError(f"debug_deform_sparse: {mw.size} morph weights for {o.size - 1} targets")
    out = np.zeros_like(r)
    po, pv, pd = sparse_pointers(o, v, d)
    rc = L.glrtx_debug_deform_sparse(_fp(r), r.shape[0], b.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), _fp(m), m.shape[0], int(mode), po, pv, pd,
                                     _fp(mw) if mw.size else None, mw.size, _fp(out))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def debug_rebuild_normals(vert, tri, class_of_vertex, flip):
    """glrtx_debug_rebuild_normals on the current device: the rebuild's three passes alone -- vert (n, 15) float32, tri (n_tri, 4) float32, a class id a vertex
    (n,) uint32 (any ids below n) and a flip byte a triangle (n_tri,) uint8.  Returns the vertices (n, 15) float32 with their normal words rebuilt."""
    from .host import _ptr, normals_arrays
    L = lib()
    v, t, c, f = normals_arrays("debug_rebuild_normals", vert, tri, class_of_vertex, flip)
    out = np.zeros_like(v)
    rc = L.glrtx_debug_rebuild_normals(_ptr(v, C.c_float), v.shape[0], _ptr(t, C.c_float), t.shape[0], _ptr(c, C.c_uint32), _ptr(f, C.c_uint8),
                                       _ptr(out, C.c_float))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return out


def _host_vertices(v, width=15, fn="update_vertices", what="vertices"):
    """A numpy array of rows for an update call: float32, shape (n, width) or flat -- 15 words a vertex for glrtx_update_vertices (or the scene's (n * 5, 3)
    texels), 3 a position for glrtx_update_positions.  Returns (array, n)."""
    a = np.asarray(v)
    if a.dtype != np.float32:
        raise TypeError(f"{fn}: float32 {what} expected, got {a.dtype}")
    if a.size % width or (a.ndim == 2 and a.shape[1] not in (3, width)) or a.ndim > 2:
        raise ValueError(f"{fn}: shape {a.shape} is not (n, {width}) or flat n * {width}")
    a = np.ascontiguousarray(a)
    return a, a.size // width


def _device_vertices(t, device_index, width=15, fn="update_vertices", what="vertices"):
    """A torch tensor of rows for the _device form of an update call: contiguous float32 on the context's GPU, shape (n, width) or flat.  Returns (pointer, n)."""
    import torch
    if t.dtype != torch.float32:
        raise TypeError(f"{fn}: float32 {what} expected, got {t.dtype}")
    if t.device.type != "cuda" or (device_index is not None and t.device.index != device_index):
        raise ValueError(f"{fn}: the tensor is on {t.device}, the context on cuda:{device_index}")
    if not t.is_contiguous():
        raise ValueError(f"{fn}: the tensor is not contiguous")
    if not (t.dim() == 1 and t.numel() % width == 0) and not (t.dim() == 2 and t.shape[1] == width):
        raise ValueError(f"{fn}: shape {tuple(t.shape)} is not (n, {width}) or flat n * {width}")
    return t.data_ptr(), t.numel() // width


def _bone_data(fn, what, data, per, shapes):
    """The bone data of a pose call: float32 with `per` words a bone.  Returns (array, n_bones)."""
    m = _f32(data)
    if m.size % per:
        raise ValueError(f"{fn}: {what} must be {shapes}, got {m.shape}")
    return m, m.size // per


_MATRIX_SHAPES = "(n_bones, 12) or (n_bones, 3, 4)"


def pack_compact(scene):
    """glrtx_debug_pack_compact (host only, no device): (records (n, 12) float32, rank table (n_words / 2, 2) uint32, 64-byte leaf records by id (n_ids, 16) float32)."""
    L = lib()
    arrs = [_f32(scene[k]) for k in ("vert", "tri", "mat", "light", "bvh")]
    args = []
    for a, w in zip(arrs, (15, 4, 18, 4, 9)):
        args += [_fp(a), a.size // w]
    n_pos, n_ids = C.c_int(), C.c_int()
    rc = L.glrtx_debug_pack_compact(*args, None, 0, C.byref(n_pos), None, 0, None, 0, C.byref(n_ids))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    recs = np.zeros((n_pos.value, 12), np.float32)
    ranks = np.zeros(((n_pos.value + 31) // 32, 2), np.uint32)
    leaves = np.zeros((n_ids.value, 16), np.float32)
    rc = L.glrtx_debug_pack_compact(*args, _fp(recs), recs.shape[0], C.byref(n_pos), ranks.ctypes.data_as(C.POINTER(C.c_uint32)), ranks.size,
                                    _fp(leaves), leaves.shape[0], C.byref(n_ids))
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(None).decode())
    return recs, ranks, leaves


def _adaptive_args(params, seeds, threshold, min_samples):
    p = params if isinstance(params, Params) else make_params(dict(params, seed=(0.0, 0.0)) if "seed" not in params else params)
    sd = _f32(np.asarray(seeds, np.float32).reshape(-1, 2))
    return p, sd, Adaptive(float(threshold), int(min_samples))


def _read_image(L, ctx, fn, *args, dtype=np.float32, planes=(), split=False):
    """What a read-back or a resolve of the context `ctx` returns: zeros of planes + (owned_rows, width, 4) of `dtype`, filled by fn(ctx, address, packed row
    pitch, *args) -- with `split`, by fn(ctx, one address per plane, pitch, *args)."""
    s = Stats()
    rc = L.glrtx_get_stats(ctx, C.byref(s))
    out = np.zeros(tuple(planes) + (s.owned_rows, s.width, 4), dtype)
    dst = [a.ctypes.data for a in out] if split else [out.ctypes.data]
    rc = rc or fn(ctx, *dst, s.width * 4 * out.itemsize, *args)
    if rc != 0:
        raise GlrtxError(rc, L.glrtx_last_error(ctx).decode())
    return out


class Device:
    """One glrtx_ctx: one GPU, one row-stripe partition of the image."""

    def __init__(self, device_id: int = -1):
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.glrtx_create(C.byref(self.h), device_id)
        if rc != 0:
            raise GlrtxError(rc, self.L.glrtx_last_error(None).decode())
        self.device_id = device_id
        self._rig_vertices = 0  # of the last upload_rig (upload_morph_targets names it when it drops the targets)

    def close(self):
        if self.h:
            self.L.glrtx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise GlrtxError(rc, self.L.glrtx_last_error(self.h).decode())

    def upload_scene(self, scene):
        v, t, m, l, b = (_f32(scene[k]) for k in ("vert", "tri", "mat", "light", "bvh"))
        self._ck(self.L.glrtx_upload_scene(self.h, _fp(v), v.size // 15, _fp(t), t.size // 4, _fp(m), m.size // 18,
                                           _fp(l), l.size // 4, _fp(b), b.size // 9))

    def _update(self, v, width, fn, what, host_call, device_call):
        """update_vertices / update_positions: a numpy array goes through `host_call`, a torch tensor through `device_call`."""
        if type(v).__module__.startswith("torch"):
            import torch
            idx = self.device_id if self.device_id >= 0 else torch.cuda.current_device()
            ptr, n = _device_vertices(v, idx, width, fn, what)
            self._ck(device_call(self.h, C.c_void_p(ptr), n))
        else:
            a, n = _host_vertices(v, width, fn, what)
            self._ck(host_call(self.h, _fp(a), n))

    def update_vertices(self, v):
        """New positions and normals for the uploaded scene's vertices, refitted on the device (glrtx_update_vertices): a numpy array is taken from host
        memory, a contiguous float32 torch tensor on the context's GPU (shape (n, 15) or flat) is read on the context's stream (glrtx_update_vertices_device:
        order its producer there with set_stream, or synchronise).  Returns when the refit has run; the accumulator is not cleared."""
        self._update(v, 15, "update_vertices", "vertices", self.L.glrtx_update_vertices, self.L.glrtx_update_vertices_device)

    def upload_normal_topology(self, rest, tri, flags=0):
        """glrtx_upload_normal_topology: the weld classes, orientation and face lists of the rest vertices (n, 15) float32 (or the scene's vertex texels) and the
        wire triangles (n_tri, 4) float32, kept on the device with a copy of the rest vertices for update_positions() and set_pose_normals().  flags: 0, or
        host.NORMALS_WELD_POSITIONS to weld by position alone."""
        r = _f32(rest).reshape(-1, 15)
        t = _f32(tri).reshape(-1, 4)
        self._ck(self.L.glrtx_upload_normal_topology(self.h, _fp(r), r.shape[0], _fp(t), t.shape[0], int(flags)))

    def update_positions(self, p):
        """New positions alone for the uploaded scene's vertices; the normals are rebuilt on the device and the tree refitted (glrtx_update_positions): a numpy
        array (n, 3) or flat is taken from host memory, a contiguous float32 torch tensor on the context's GPU is read on the context's stream
        (glrtx_update_positions_device), as update_vertices does.  Needs upload_normal_topology.  Returns when the refit has run."""
        self._update(p, 3, "update_positions", "positions", self.L.glrtx_update_positions, self.L.glrtx_update_positions_device)

    def set_pose_normals(self, enable=True):
        """glrtx_set_pose_normals: while on, pose / pose_morph / pose_dualquat rebuild the normals between their kernel and the refit."""
        self._ck(self.L.glrtx_set_pose_normals(self.h, 1 if enable else 0))

    def normals_burst_ms(self, reps=20) -> float:
        """glrtx_debug_normals_burst: device ms of one rebuild (its three passes on the vertex buffer), from `reps` back to back."""
        ms = C.c_float(0)
        self._ck(self.L.glrtx_debug_normals_burst(self.h, int(reps), C.byref(ms)))
        return float(ms.value)

    def upload_rig(self, rest, bones, weights, n_bones):
        """glrtx_upload_rig: the rest pose (n, 15) float32 (or the scene's vertex texels), four bone indices (n, 4) int32 and four weights (n, 4) float32 a
        vertex, kept on the device for pose().  glrt_amd.rig.rigid gives the bones and weights of rigid objects."""
        from .host import rig_arrays
        r, b, w = rig_arrays("upload_rig", rest, bones, weights)
        self._ck(self.L.glrtx_upload_rig(self.h, _fp(r), r.shape[0], b.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), int(n_bones)))
        self._rig_vertices = r.shape[0]

    def pose(self, matrices):
        """glrtx_pose: matrices (n_bones, 12) float32, row-major 3x4 -- skins the rest pose on the device and refits, as update_vertices of the skinned
        vertices would.  Returns when the refit has run; the accumulator is not cleared."""
        m, n_bones = _bone_data("pose", "matrices", matrices, 12, _MATRIX_SHAPES)
        self._ck(self.L.glrtx_pose(self.h, _fp(m), n_bones))

    def upload_morph_targets(self, deltas):
        """glrtx_upload_morph_targets: deltas (n_targets, n_vert, 6) float32 {dpos, dnormal} for the uploaded rig; None or an empty array drops the targets."""
        d = np.zeros((0, 0, 6), np.float32) if deltas is None else _f32(deltas)
        if d.ndim != 3 or d.shape[2] != 6:
            raise ValueError(f"upload_morph_targets: deltas must be (n_targets, n_vert, 6), got {d.shape}")
        if d.shape[0] == 0:  # dropping: the call still names the rig's vertex count
            self._ck(self.L.glrtx_upload_morph_targets(self.h, None, 0, self._rig_vertices))
        else:
            self._ck(self.L.glrtx_upload_morph_targets(self.h, _fp(d), d.shape[0], d.shape[1]))

    def upload_morph_targets_sparse(self, offsets, vertex=None, deltas=None, n_vert=None):
        """glrtx_upload_morph_targets_sparse: a sparse set for the uploaded rig -- offsets (n_targets + 1,) uint64, vertex (nnz,) uint32, deltas (nnz, 6) float32
        {dpos, dnormal} (glrt_amd.host.morph_sparsify makes the three from dense deltas).  offsets None, or a single 0, drops whatever set the rig holds.
        n_vert: the vertex count the set was made for (the rig's, unless given)."""
        from .host import sparse_arrays, sparse_pointers
        o, v, d = sparse_arrays("upload_morph_targets_sparse", offsets, vertex, deltas)
        po, pv, pd = sparse_pointers(o, v, d)
        self._ck(self.L.glrtx_upload_morph_targets_sparse(self.h, po, pv, pd, o.size - 1, self._rig_vertices if n_vert is None else int(n_vert)))

    @staticmethod
    def _morph_weights(w):
        mw = np.zeros(0, np.float32) if w is None else _f32(w).reshape(-1)
        return (_fp(mw) if mw.size else None), mw.size, mw

    def pose_morph(self, matrices, morph_weights=None):
        """glrtx_pose_morph: pose() with one weight a morph target of the rig (None: the rig has none)."""
        m, n_bones = _bone_data("pose_morph", "matrices", matrices, 12, _MATRIX_SHAPES)
        p, n, keep = self._morph_weights(morph_weights)
        self._ck(self.L.glrtx_pose_morph(self.h, _fp(m), n_bones, p, n))

    def pose_dualquat(self, dualquats, morph_weights=None):
        """glrtx_pose_dualquat: dualquats (n_bones, 8) float32 {r.xyzw, d.xyzw} (glrt_amd.rig.dualquat), and the morph weights as for pose_morph."""
        q, n_bones = _bone_data("pose_dualquat", "dual quaternions", dualquats, 8, "(n_bones, 8)")
        p, n, keep = self._morph_weights(morph_weights)
        self._ck(self.L.glrtx_pose_dualquat(self.h, _fp(q), n_bones, p, n))

    def deform_burst_ms(self, reps=20) -> float:
        """glrtx_debug_deform_burst: device ms of one launch of the deform kernel (the last pose_morph / pose_dualquat again), from `reps` back to back."""
        ms = C.c_float(0)
        self._ck(self.L.glrtx_debug_deform_burst(self.h, int(reps), C.byref(ms)))
        return float(ms.value)

    def skin_burst_ms(self, reps=20) -> float:
        """glrtx_debug_skin_burst: device ms of one launch of the skinning kernel (the rig with the last pose's matrices), from `reps` launches back to back."""
        ms = C.c_float(0)
        self._ck(self.L.glrtx_debug_skin_burst(self.h, int(reps), C.byref(ms)))
        return float(ms.value)

    def trace_rays(self, rays, any_hit=False, out=None):
        """Batched ray queries against the uploaded scene (glrtx_trace_rays, include/glrtx.h).  rays: (n, 8) float32 {ox, oy, oz, tmin, dx, dy, dz, tmax}.
        Closest hit, or with any_hit=True the first accepted hit of the renderer's visiting order.  Returns (t, tri, u, v): views of one (n, 4) buffer, tri as
        int32 (the wire triangle index; -1 on a miss, where t = tmax and u = v = 0).
          numpy array  -> host memory (glrtx_trace_rays); returns when the hits are there.  out: an (n, 4) float32 array, or None.
          torch tensor -> contiguous float32 on the context's GPU, read and written on the context's stream with no host copy (glrtx_trace_rays_device),
                          the convention of update_vertices: order the producer of `rays` there (set_stream) or synchronise, and wait on that stream
                          (or sync()) before reading the result.  out: an (n, 4) float32 CUDA tensor, or None for a new one (allocated on torch's
                          current stream).  Returns as soon as the query is enqueued."""
        flags = 1 if any_hit else 0
        if type(rays).__module__.startswith("torch"):
            import torch
            idx = self.device_id if self.device_id >= 0 else torch.cuda.current_device()
            if rays.dtype != torch.float32 or rays.device.type != "cuda" or rays.device.index != idx or not rays.is_contiguous():
                raise ValueError(f"trace_rays: a contiguous float32 tensor on cuda:{idx} expected, got {rays.dtype} on {rays.device}")
            if rays.numel() % 8:
                raise ValueError(f"trace_rays: shape {tuple(rays.shape)} is not (n, 8)")
            n = rays.numel() // 8
            if out is None:
                out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
            elif out.dtype != torch.float32 or out.device != rays.device or not out.is_contiguous() or out.numel() != 4 * n:
                raise ValueError("trace_rays: out must be a contiguous (n, 4) float32 tensor on the rays' device")
            out = out.view(n, 4)
            self._ck(self.L.glrtx_trace_rays_device(self.h, C.c_void_p(rays.data_ptr()), n, C.c_void_p(out.data_ptr()), flags))
            return out[:, 0], out[:, 1].view(torch.int32), out[:, 2], out[:, 3]
        r = _f32(rays).reshape(-1, 8)
        n = r.shape[0]
        if out is None:
            out = np.zeros((n, 4), np.float32)
        elif out.dtype != np.float32 or not out.flags.c_contiguous or out.size != 4 * n:
            raise ValueError("trace_rays: out must be a C-contiguous (n, 4) float32 array")
        out = out.reshape(n, 4)
        self._ck(self.L.glrtx_trace_rays(self.h, _fp(r), n, _fp(out), flags))
        return out[:, 0], out[:, 1].view(np.int32), out[:, 2], out[:, 3]

    def read_scene(self, which) -> np.ndarray:
        """glrtx_debug_read_scene: one device scene buffer ("nodes", "cnodes", "nrms", "lights", "vine", "root") as raw bytes (uint8)."""
        k = SCENE_BUFFERS.index(which)
        n = C.c_size_t(0)
        self._ck(self.L.glrtx_debug_read_scene(self.h, k, None, 0, C.byref(n)))
        out = np.zeros(max(int(n.value), 1), np.uint8)
        self._ck(self.L.glrtx_debug_read_scene(self.h, k, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out[:int(n.value)]

    def build_lbvh(self, vert, tri):
        """Linear BVH built on the GPU.  Returns (nodes (n_nodes*3, 3) float32 in the wire format, max_depth, device ms)."""
        v, t = _f32(vert).reshape(-1, 15), _f32(tri).reshape(-1, 4)
        nodes = np.zeros(((2 * t.shape[0] - 1) * 3, 3), np.float32)
        depth, ms = C.c_int(0), C.c_float(0)
        self._ck(self.L.glrtx_build_lbvh(self.h, _fp(v), v.shape[0], _fp(t), t.shape[0], _fp(nodes), C.byref(depth), C.byref(ms)))
        return nodes, int(depth.value), float(ms.value)

    def build_bvh_sah(self, vert, tri):
        """Binned SAH by levels + exact sweep at the bottom, built on the GPU (glrtx_build_bvh_sah).  Returns (nodes, max_depth, device ms) like build_lbvh."""
        v, t = _f32(vert).reshape(-1, 15), _f32(tri).reshape(-1, 4)
        nodes = np.zeros(((2 * t.shape[0] - 1) * 3, 3), np.float32)
        depth, ms = C.c_int(0), C.c_float(0)
        self._ck(self.L.glrtx_build_bvh_sah(self.h, _fp(v), v.shape[0], _fp(t), t.shape[0], _fp(nodes), C.byref(depth), C.byref(ms)))
        return nodes, int(depth.value), float(ms.value)

    def upload_spheres(self, spheres):
        """EXTENSION (parity unpinned): (n, 5) rows [cx, cy, cz, radius, material]; None or empty removes them."""
        sp = _f32(np.zeros((0, 5)) if spheres is None else np.asarray(spheres, np.float32).reshape(-1, 5))
        self._ck(self.L.glrtx_upload_spheres(self.h, _fp(sp), sp.shape[0]))

    def upload_textures(self, textures, material_texture):
        """Bind a texture set (glrtx_upload_textures; include/glrtx.h "Textures"): textures as host.pack_textures takes them -- a list of (array, format, wrap,
        filter) --, material_texture one texture index a material of the uploaded scene (-1: untextured; only diffuse materials can be bound).  Launches then run
        on the extension megakernel (or, with set_texture_wavefront, on the wavefront kernel's T form).  None or an empty list unbinds.  The triangles' texture coordinates are those of the uploaded scene's vertices, frozen."""
        from .host import pack_textures
        desc, blob = pack_textures(textures or [])
        b = np.ascontiguousarray([] if material_texture is None else material_texture, dtype=np.int32).reshape(-1)
        self._ck(self.L.glrtx_upload_textures(self.h, desc.ctypes.data, desc.size, blob.ctypes.data, blob.size, b.ctypes.data_as(C.POINTER(C.c_int32)), b.size))

    def bind_material_maps(self, normal=None, roughness=None, normal_scale=1.0):
        """Bind material maps on top of the bound texture set (glrtx_bind_material_maps; include/glrtx.h "Material maps"): per-material arrays of texture
        indices (-1: none) and normal-map scales, or one array of host.MATERIAL_MAP_DTYPE records as `normal`.  A normal map goes on a diffuse or conductor
        material, a roughness map on a conductor.  Both None unbinds.  upload_textures and upload_scene drop the maps."""
        from .host import MATERIAL_MAP_DTYPE, material_maps
        if normal is None and roughness is None:
            self._ck(self.L.glrtx_bind_material_maps(self.h, None, 0))
            return
        if getattr(normal, "dtype", None) == MATERIAL_MAP_DTYPE:
            rec = np.ascontiguousarray(normal).reshape(-1)
        else:
            rec = material_maps(np.size(normal if normal is not None else roughness), normal, roughness, normal_scale)
        self._ck(self.L.glrtx_bind_material_maps(self.h, rec.ctypes.data, rec.size))

    def bind_cutouts(self, texture=None, channel=None, cutoff=None):
        """Bind alpha cutouts on top of the bound texture set (glrtx_bind_cutouts; include/glrtx.h "Cutouts"): per-material arrays of texture indices (-1:
        not cut), channels (0 .. 3; default 3, alpha) and cutoffs (default 0.5), or one array of host.CUTOUT_DTYPE records as `texture`.  A candidate hit on a
        bound diffuse or conductor material counts only where the channel's value >= cutoff -- for path and shadow rays alike.  Launches then run on the
        extension megakernel's CUT forms.  texture None unbinds.  upload_textures and upload_scene drop the records; vertex updates and poses keep them."""
        from .host import CUTOUT_DTYPE, cutouts
        if texture is None:
            self._ck(self.L.glrtx_bind_cutouts(self.h, None, 0))
            return
        if getattr(texture, "dtype", None) == CUTOUT_DTYPE:
            rec = np.ascontiguousarray(texture).reshape(-1)
        else:
            rec = cutouts(np.size(texture), texture, channel, cutoff)
        self._ck(self.L.glrtx_bind_cutouts(self.h, rec.ctypes.data, rec.size))

    def bind_emission_maps(self, material_emission=None):
        """Bind emission maps on top of the bound texture set (glrtx_bind_emission_maps; include/glrtx.h "Emission maps"): one texture index a material (-1:
        none; any type but media).  A bound emitter's radiance is emission * texel, where it is seen and where next-event estimation samples it.  Launches
        then run on the extension megakernel's emission-map forms.  None unbinds.  upload_textures and upload_scene drop the bindings; vertex updates and
        poses keep them."""
        if material_emission is None:
            self._ck(self.L.glrtx_bind_emission_maps(self.h, None, 0))
            return
        b = np.ascontiguousarray(material_emission, dtype=np.int32).reshape(-1)
        self._ck(self.L.glrtx_bind_emission_maps(self.h, b.ctypes.data_as(C.POINTER(C.c_int32)), b.size))

    def debug_light_emission(self, lid, u):
        """glrtx_debug_light_emission: (n, 5) float32 {s, t, Le.rgb} of light lid[i] at the raw uniforms u[i] (see device.debug_light_emission)."""
        k = np.ascontiguousarray(lid, dtype=np.int32).reshape(-1)
        uu = _f32(u).reshape(-1, 2)
        if uu.shape[0] != k.size:
            raise ValueError(f"debug_light_emission: {k.size} lights, {uu.shape[0]} uniform pairs")
        out = np.zeros((k.size, 5), np.float32)
        self._ck(self.L.glrtx_debug_light_emission(self.h, k.ctypes.data_as(C.POINTER(C.c_int32)), _fp(uu), k.size, _fp(out)))
        return out

    def last_kernel(self) -> str:
        """glrtx_debug_last_kernel: the name of the render kernel the last launch ran, as error reports give it ("" before the first launch)."""
        return self.L.glrtx_debug_last_kernel(self.h).decode()

    def upload_environment(self, env_map, cfg=None):
        """Bind an environment (glrtx_upload_environment; include/glrtx.h "Environment"): env_map as host.pack_environment takes it -- (array (N, N, 3 or 4),
        format, filter), an octahedral map with +y at the centre --, cfg a device.EnvCfg (host.env_cfg builds one; default: escape mode, scale 1, no rotation).
        Launches then run on the extension megakernel.  env_map None unbinds.  The map is kept across upload_scene."""
        from .host import env_cfg, pack_environment
        if env_map is None:
            self._ck(self.L.glrtx_upload_environment(self.h, None, None, 0, None))
            return
        cfg = env_cfg() if cfg is None else cfg
        desc, blob = pack_environment(env_map)
        self._ck(self.L.glrtx_upload_environment(self.h, desc.ctypes.data, blob.ctypes.data, blob.size, C.addressof(cfg)))

    def set_environment_cfg(self, cfg):
        """glrtx_set_environment_cfg: mode, light_pick and rotation take effect at the next launch; a new scale or grid rebuilds the sampling tables."""
        self._ck(self.L.glrtx_set_environment_cfg(self.h, C.addressof(cfg) if cfg is not None else None))

    def set_extensions(self, flags: int):
        """EXT_DIELECTRIC | EXT_WHITTED (extensions, parity unpinned) | EXT_VOLUME (the reference's volume branch, pinned)."""
        self._ck(self.L.glrtx_set_extensions(self.h, int(flags)))

    def upload_volume(self, density, temperature, bbox_min, bbox_max, density_max=None):
        """The volume of the media materials (glrtx_upload_volume): density / temperature grids shaped (nz, ny, nx) -- x fastest, as
        glTexSubImage3D reads them -- and the bbox from the scene.  density_max defaults to the density grid's maximum (the reference takes
        the maximum over the whole file).  density None removes the volume.  Rendering needs EXT_VOLUME (set_extensions) as well."""
        self._ck(_upload_volume(self.L.glrtx_upload_volume, self.h, density, temperature, bbox_min, bbox_max, density_max))

    def set_volume_wavefront(self, enable: bool):
        """True: volume launches (EXT_VOLUME alone) run on the wavefront kernel's V form -- frames in flight, fed launches, the present ring and
        render_adaptive with the volume on; bit-identical to the persistent megakernel (the default).  GLRTX_VOLUME_WAVEFRONT=0/1 overrides it per launch."""
        self._ck(self.L.glrtx_set_volume_wavefront(self.h, int(enable)))

    def set_texture_wavefront(self, enable: bool):
        """True: launches with a texture set bound (material maps included) and nothing else that needs the extension kernel run on the wavefront
        kernel's T / TM forms -- frames in flight, fed launches, the present ring, render_adaptive*, render_moments and render_cascades with the set
        bound; bit-identical to the textured megakernel (the default).  GLRTX_TEXTURE_WAVEFRONT=0/1 overrides it per launch."""
        self._ck(self.L.glrtx_set_texture_wavefront(self.h, int(enable)))

    def set_partition(self, rank, world, stripe_rows=16):
        self._ck(self.L.glrtx_set_partition(self.h, rank, world, stripe_rows))

    def resize(self, w, h):
        self._ck(self.L.glrtx_resize(self.h, w, h))

    def clear(self):
        self._ck(self.L.glrtx_clear(self.h))

    def bind_accum(self, device_ptr, pitch_bytes, capacity_rows):
        self._ck(self.L.glrtx_bind_accum(self.h, C.c_void_p(device_ptr), pitch_bytes, int(capacity_rows)))

    def set_stream(self, hip_stream):
        self._ck(self.L.glrtx_set_stream(self.h, C.c_void_p(hip_stream)))

    def set_variant(self, variant: int):
        self._ck(self.L.glrtx_set_variant(self.h, int(variant)))

    def set_shadow_range_limit(self, enable: bool):
        """False (default): shadow rays are searched like the reference's; True: with the range limit of rounds 1-4 (faster, not part of the bit-exact contract)."""
        self._ck(self.L.glrtx_set_shadow_range_limit(self.h, int(enable)))

    def count_rays(self, enable=True):
        self._ck(self.L.glrtx_count_rays(self.h, int(enable)))

    def render(self, params):
        p = params if isinstance(params, Params) else make_params(params)
        self._ck(self.L.glrtx_render(self.h, C.byref(p)))

    def render_frames(self, params, seeds):
        """Frames in flight: len(seeds) consecutive frames that differ only in u_seed, as one launch."""
        p = params if isinstance(params, Params) else make_params(dict(params, seed=(0.0, 0.0)) if "seed" not in params else params)
        sd = _f32(np.asarray(seeds, np.float32).reshape(-1, 2))
        self._ck(self.L.glrtx_render_frames(self.h, C.byref(p), _fp(sd), sd.shape[0]))

    def sync(self):
        self._ck(self.L.glrtx_sync(self.h))

    def stats(self) -> Stats:
        s = Stats()
        self._ck(self.L.glrtx_get_stats(self.h, C.byref(s)))
        return s

    def reset_stats(self):
        self._ck(self.L.glrtx_reset_stats(self.h))

    def local_rows_y(self):
        n = self.stats().owned_rows
        return np.array([self.L.glrtx_local_row_to_y(self.h, r) for r in range(n)], np.int64)

    def read_accum(self) -> np.ndarray:
        return _read_image(self.L, self.h, self.L.glrtx_read_accum)

    def resolve_rgba8(self, gamma=2.2, flip_y=True) -> np.ndarray:
        return _read_image(self.L, self.h, self.L.glrtx_resolve_rgba8, gamma, int(flip_y), dtype=np.uint8)

    def hit_histogram(self, params, n_tri) -> np.ndarray:
        """Closest hits per triangle of the uploaded scene in ONE calibration frame of `params` (glrtx_hit_histogram): input of host.order_by_hits."""
        p = params if isinstance(params, Params) else make_params(params)
        out = np.zeros(int(n_tri), np.uint32)
        self._ck(self.L.glrtx_hit_histogram(self.h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint32)), int(n_tri)))
        return out

    def resolve_burst_ms(self, gamma=2.2, reps=32) -> float:
        """Device time of one launch of the resolve kernel, from `reps` launches back to back (glrtx_debug_resolve_burst)."""
        ms = C.c_float(0)
        self._ck(self.L.glrtx_debug_resolve_burst(self.h, gamma, int(reps), C.byref(ms)))
        return float(ms.value)

    def present_enable(self, ring, gamma=2.2, flip_y=True):
        """Every frame's image into a ring of `ring` pinned RGBA8 images (glrtx_present_enable); ring = 0 turns it off (untaken images are dropped)."""
        self._ck(self.L.glrtx_present_enable(self.h, int(ring), gamma, int(flip_y)))

    def present_acquire(self, wait=True):
        """The oldest image not yet acquired: a Presented (.frame, .rgba zero-copy view), or None when wait=False and it is not ready (GLRTX_EBUSY)."""
        img = Image()
        rc = self.L.glrtx_present_acquire(self.h, int(wait), C.byref(img))
        if rc == GLRTX_EBUSY and not wait:
            return None
        self._ck(rc)
        return Presented(img)

    def present_release(self, img):
        self._ck(self.L.glrtx_present_release(self.h, C.byref(img.img)))

    def present_stats(self) -> PresentStats:
        s = PresentStats()
        self._ck(self.L.glrtx_present_get_stats(self.h, C.byref(s)))
        return s

    def render_adaptive(self, params, seeds, threshold, min_samples=2):
        """Adaptive sampling (glrtx_render_adaptive): select the active 8x8 tiles, then render len(seeds) frames of those tiles only.  threshold < 0: nothing retires."""
        p, sd, cfg = _adaptive_args(params, seeds, threshold, min_samples)
        self._ck(self.L.glrtx_render_adaptive(self.h, C.byref(p), _fp(sd), sd.shape[0], C.byref(cfg)))
    def render_adaptive_moments(self, params, seeds, cfg, min_samples=2):
        """render_adaptive with the selection made from the moments plane M and the active tiles' samples folded into M (glrtx_render_adaptive_moments; needs
        track_moments).  cfg: an Adaptive, or the threshold (then min_samples applies).  Its thresholds are not render_adaptive's: here a tile's error is the
        mean standard error of its pixels' mean luminance over the root of that luminance.  The half buffer is neither read nor written."""
        if isinstance(cfg, Adaptive):
            cfg, min_samples = cfg.threshold, cfg.min_samples
        p, sd, k = _adaptive_args(params, seeds, cfg, min_samples)
        self._ck(self.L.glrtx_render_adaptive_moments(self.h, C.byref(p), _fp(sd), sd.shape[0], C.byref(k)))
    def adaptive_active_tiles(self):
        """(active, total) tiles of the last selection (syncs)."""
        a, t = C.c_int(0), C.c_int(0)
        self._ck(self.L.glrtx_adaptive_active_tiles(self.h, C.byref(a), C.byref(t)))
        return int(a.value), int(t.value)
    def tile_mask(self) -> np.ndarray:
        """The last selection's mask, (tiles_y, tiles_x) uint8 over the owned rows (syncs)."""
        s = self.stats()
        out = np.zeros(((s.owned_rows + 7) // 8, (s.width + 7) // 8), np.uint8)
        self._ck(self.L.glrtx_read_tile_mask(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out
    def read_adaptive_half(self) -> np.ndarray:
        """The half buffer H (every second sample), (owned_rows, width, 4) float32 like read_accum."""
        return _read_image(self.L, self.h, self.L.glrtx_read_adaptive_half)
    def render_features(self, params):
        """The denoiser's feature planes for this camera (glrtx_render_features): issued on the context's stream, nothing is read back."""
        p = make_params(params)
        self._ck(self.L.glrtx_render_features(self.h, C.byref(p)))
    def read_features(self):
        """(normal_depth, albedo_id): (owned_rows, width, 4) float32 each (syncs); albedo_id[..., 3] holds the material id as int32 bits, -1 on a miss."""
        n, a = _read_image(self.L, self.h, self.L.glrtx_read_features, planes=(2,), split=True)
        return n, a
    def denoise(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None):
        """The a-trous filter over the accumulator's mean, guided by the feature planes as they stand (glrtx_denoise); None: the default."""
        c = denoise_cfg(iterations, sigma_color, sigma_normal, sigma_depth, demodulate)
        self._ck(self.L.glrtx_denoise(self.h, C.byref(c)))
    def read_denoised(self) -> np.ndarray:
        """The denoised image D, (owned_rows, width, 4) float32 {rgb, 1} (syncs)."""
        return _read_image(self.L, self.h, self.L.glrtx_read_denoised)
    def resolve_denoised_rgba8(self, gamma=2.2, flip_y=True) -> np.ndarray:
        return _read_image(self.L, self.h, self.L.glrtx_resolve_denoised_rgba8, gamma, int(flip_y), dtype=np.uint8)
    def track_moments(self, enable=True):
        """Keep the luminance moments plane M beside the accumulator (glrtx_track_moments); off by default, switching it off releases M."""
        self._ck(self.L.glrtx_track_moments(self.h, int(bool(enable))))
    def render_moments(self, params, seeds):
        """render_frames that also folds every sample's luminance and squared luminance into M (glrtx_render_moments); the accumulator is render_frames'."""
        p = params if isinstance(params, Params) else make_params(dict(params, seed=(0.0, 0.0)) if "seed" not in params else params)
        sd = _f32(np.asarray(seeds, np.float32).reshape(-1, 2))
        self._ck(self.L.glrtx_render_moments(self.h, C.byref(p), _fp(sd), sd.shape[0]))
    def read_moments(self) -> np.ndarray:
        """The moments plane M {sum l, sum l^2, 0, count}, (owned_rows, width, 4) float32 like read_accum (syncs)."""
        return _read_image(self.L, self.h, self.L.glrtx_read_moments)
    def denoise_variance(self, iterations=None, sigma_lum=None, sigma_normal=None, sigma_depth=None, demodulate=None):
        """The variance-guided a-trous filter over the accumulator's mean, steered by M and the feature planes as they stand (glrtx_denoise_variance); the result
        is read with read_denoised / resolve_denoised_rgba8.  None: the default."""
        c = denoise_var_cfg(iterations, sigma_lum, sigma_normal, sigma_depth, demodulate)
        self._ck(self.L.glrtx_denoise_variance(self.h, C.byref(c)))
    def track_cascades(self, enable=True, start=None):
        """Keep the six luminance cascade planes C beside the accumulator, with bounds start * 8^k (glrtx_track_cascades); off by default, switching it off
        releases C, another start zeroes it."""
        from .host import REWEIGHT_DEFAULTS
        self._ck(self.L.glrtx_track_cascades(self.h, int(bool(enable)), float(REWEIGHT_DEFAULTS["start"] if start is None else start)))
    def render_cascades(self, params, seeds):
        """render_frames that also splits every sample by luminance over the cascade planes C (glrtx_render_cascades); the accumulator is render_frames'."""
        p = params if isinstance(params, Params) else make_params(dict(params, seed=(0.0, 0.0)) if "seed" not in params else params)
        sd = _f32(np.asarray(seeds, np.float32).reshape(-1, 2))
        self._ck(self.L.glrtx_render_cascades(self.h, C.byref(p), _fp(sd), sd.shape[0]))
    def read_cascades(self) -> np.ndarray:
        """The cascade planes C {sum w r, sum w g, sum w b, count}, (6, owned_rows, width, 4) float32 (syncs)."""
        return _read_image(self.L, self.h, self.L.glrtx_read_cascades, planes=(6,))
    def reweight(self, cfg=None, kappa=None):
        """The firefly re-weighting resolve of C into the image D (glrtx_reweight); the result is read with read_denoised / resolve_denoised_rgba8 and is
        source = 1 of the tone-mapping and bloom calls.  None: the default."""
        k = cfg if cfg is not None else reweight_cfg(kappa)
        self._ck(self.L.glrtx_reweight(self.h, C.byref(k)))
    def reweight_burst_ms(self, reps=20, cfg=None, kappa=None) -> float:
        k = cfg if cfg is not None else reweight_cfg(kappa)
        ms = C.c_float()
        self._ck(self.L.glrtx_debug_reweight_burst(self.h, C.byref(k), int(reps), C.byref(ms)))
        return float(ms.value)
    def reproject(self, params, max_history=None, depth_tolerance=None, normal_tolerance=None):
        """Carry the accumulator from the camera of the last render_features / reproject to `params`' camera (glrtx_reproject); None: the default.  The
        accumulator's device address changes; the feature planes are `params`' afterwards."""
        p = make_params(params)
        c = ReprojectCfg.default(max_history, depth_tolerance, normal_tolerance)
        self._ck(self.L.glrtx_reproject(self.h, C.byref(p), C.byref(c)))
    def reproject_last(self):
        """(carried, hit_pixels) of the last reproject (syncs)."""
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self.L.glrtx_reproject_last(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)
    def track_motion(self, enable=True):
        """Motion tracking on or off (glrtx_track_motion): while on, the feature passes also write the geometry plane and update_vertices keeps the geometry
        of the last feature pass, which reproject_motion needs."""
        self._ck(self.L.glrtx_track_motion(self.h, int(bool(enable))))
    def read_features_geom(self) -> np.ndarray:
        """The geometry plane G, (owned_rows, width, 4) float32 (syncs): [..., 0] the wire triangle index as int32 bits (-1: a miss), [..., 1:3] the hit's
        barycentrics."""
        return _read_image(self.L, self.h, self.L.glrtx_read_features_geom)
    def reproject_motion(self, params, max_history=None, depth_tolerance=None, normal_tolerance=None):
        """Device.reproject for geometry that update_vertices moved since the last feature pass (glrtx_reproject_motion; needs track_motion)."""
        p = make_params(params)
        c = ReprojectCfg.default(max_history, depth_tolerance, normal_tolerance)
        self._ck(self.L.glrtx_reproject_motion(self.h, C.byref(p), C.byref(c)))
    def exposure_measure(self, cfg=None, **fields):
        """One exposure measurement of the cfg's source (glrtx_exposure_measure): histogram and reduce on the context's stream, E updated on the device; no sync.
        cfg: a TonemapCfg, or its fields as keywords (None: glrt_amd.host.TONEMAP_DEFAULTS)."""
        self._ck(self.L.glrtx_exposure_measure(self.h, C.byref(_tonemap_cfg(cfg, fields))))
    def exposure_reset(self):
        """Forget E (glrtx_exposure_reset): the next measurement jumps to its target."""
        self._ck(self.L.glrtx_exposure_reset(self.h))
    def read_exposure(self) -> Exposure:
        """The last measurement (syncs): an Exposure; measurements == 0 before the first one."""
        e = Exposure()
        self._ck(self.L.glrtx_read_exposure(self.h, C.byref(e)))
        return e
    def tonemap(self, cfg=None, **fields):
        """The tone curve over the cfg's source into the context's plane T (glrtx_tonemap); no sync."""
        self._ck(self.L.glrtx_tonemap(self.h, C.byref(_tonemap_cfg(cfg, fields))))
    def read_tonemapped(self) -> np.ndarray:
        """The plane T, (owned_rows, width, 4) float32 {y.rgb, 1} (syncs)."""
        return _read_image(self.L, self.h, self.L.glrtx_read_tonemapped)
    def resolve_tonemapped_rgba8(self, cfg=None, **fields) -> np.ndarray:
        """The cfg's source through the curve and the resolve in one pass (glrtx_resolve_tonemapped_rgba8): (owned_rows, width, 4) uint8."""
        return _read_image(self.L, self.h, self.L.glrtx_resolve_tonemapped_rgba8, C.byref(_tonemap_cfg(cfg, fields)), dtype=np.uint8)
    def tonemap_burst_ms(self, which, reps=20, cfg=None, **fields) -> float:
        """Device time of one launch of a tone-mapping pass from `reps` launches back to back (glrtx_debug_tonemap_burst).  which: 0 the plain resolve kernel,
        1 the fused tone-mapping resolve, 2 the plane kernel, 3 a measurement."""
        ms = C.c_float(0)
        self._ck(self.L.glrtx_debug_tonemap_burst(self.h, C.byref(_tonemap_cfg(cfg, fields)), int(which), int(reps), C.byref(ms)))
        return float(ms.value)
    def bloom(self, cfg=None, **fields):
        """The glow of the cfg's source into the context's plane B (glrtx_bloom): 2 * levels launches on the context's stream; no sync.  cfg: a BloomCfg, or its
        fields as keywords (None: glrt_amd.host.BLOOM_DEFAULTS)."""
        self._ck(self.L.glrtx_bloom(self.h, C.byref(_bloom_cfg(cfg, fields))))
    def read_bloomed(self) -> np.ndarray:
        """The plane B, (owned_rows, width, 4) float32 {x + strength * glow, 1} (syncs)."""
        return _read_image(self.L, self.h, self.L.glrtx_read_bloomed)
    def tonemap_bloomed(self, cfg=None, **fields):
        """The tone curve over B into the context's plane T (glrtx_tonemap_bloomed; the cfg's source is not read); no sync."""
        self._ck(self.L.glrtx_tonemap_bloomed(self.h, C.byref(_tonemap_cfg(cfg, fields))))
    def resolve_bloomed_rgba8(self, cfg=None, **fields) -> np.ndarray:
        """B through the curve and the resolve in one pass (glrtx_resolve_bloomed_rgba8; the cfg's source is not read): (owned_rows, width, 4) uint8."""
        return _read_image(self.L, self.h, self.L.glrtx_resolve_bloomed_rgba8, C.byref(_tonemap_cfg(cfg, fields)), dtype=np.uint8)
    def bloom_burst_ms(self, reps=20, cfg=None, **fields) -> float:
        """Device time of one glrtx_bloom from `reps` of them back to back (glrtx_debug_bloom_burst)."""
        ms = C.c_float(0)
        self._ck(self.L.glrtx_debug_bloom_burst(self.h, C.byref(_bloom_cfg(cfg, fields)), int(reps), C.byref(ms)))
        return float(ms.value)
    def timer_begin(self):
        self._ck(self.L.glrtx_timer_begin(self.h))

    def timer_end(self) -> float:
        ms = C.c_float(0)
        self._ck(self.L.glrtx_timer_end(self.h, C.byref(ms)))
        return float(ms.value)


class Group:
    """glrtx_group: one context per listed HIP device (an ordinal may repeat), the image rows in interleaved 8-row stripes;
    read_accum / resolve_rgba8 return the FULL image, gathered on the first device."""

    def __init__(self, device_ids):
        self.L = lib()
        self.h = C.c_void_p()
        ids = (C.c_int * len(device_ids))(*device_ids)
        rc = self.L.glrtx_group_create(C.byref(self.h), ids, len(device_ids))
        if rc != 0:
            raise GlrtxError(rc, self.L.glrtx_group_last_error(None).decode())
        self.w = self.hgt = 0

    def close(self):
        if self.h:
            self.L.glrtx_group_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise GlrtxError(rc, self.L.glrtx_group_last_error(self.h).decode())

    def size(self):
        return int(self.L.glrtx_group_size(self.h))

    def member_call(self, fn, *args):
        """fn(ctx, *args) on every member (glrtx_count_rays, glrtx_set_variant, ...)."""
        for i in range(self.size()):
            rc = fn(self.L.glrtx_group_ctx(self.h, i), *args)
            if rc != 0:
                raise GlrtxError(rc, self.L.glrtx_last_error(self.L.glrtx_group_ctx(self.h, i)).decode())

    def upload_volume(self, density, temperature, bbox_min, bbox_max, density_max=None):
        """Device.upload_volume on every member (glrtx_group_upload_volume)."""
        self._ck(_upload_volume(self.L.glrtx_group_upload_volume, self.h, density, temperature, bbox_min, bbox_max, density_max))

    def upload_scene(self, scene):
        v, t, m, l, b = (_f32(scene[k]) for k in ("vert", "tri", "mat", "light", "bvh"))
        self._ck(self.L.glrtx_group_upload_scene(self.h, _fp(v), v.size // 15, _fp(t), t.size // 4, _fp(m), m.size // 18,
                                                 _fp(l), l.size // 4, _fp(b), b.size // 9))

    def update_vertices(self, v):
        """Device.update_vertices (host memory) on every member: glrtx_group_update_vertices."""
        a, n = _host_vertices(v)
        self._ck(self.L.glrtx_group_update_vertices(self.h, _fp(a), n))

    def resize(self, w, h):
        self._ck(self.L.glrtx_group_resize(self.h, w, h))
        self.w, self.hgt = w, h

    def clear(self):
        self._ck(self.L.glrtx_group_clear(self.h))

    def render(self, params):
        p = params if isinstance(params, Params) else make_params(params)
        self._ck(self.L.glrtx_group_render(self.h, C.byref(p)))

    def render_frames(self, params, seeds):
        p = params if isinstance(params, Params) else make_params(dict(params, seed=(0.0, 0.0)) if "seed" not in params else params)
        sd = _f32(np.asarray(seeds, np.float32).reshape(-1, 2))
        self._ck(self.L.glrtx_group_render_frames(self.h, C.byref(p), _fp(sd), sd.shape[0]))

    def sync(self):
        self._ck(self.L.glrtx_group_sync(self.h))
    def render_adaptive(self, params, seeds, threshold, min_samples=2):
        """Device.render_adaptive on every member, each selecting on its own accumulator (glrtx_group_render_adaptive)."""
        p, sd, cfg = _adaptive_args(params, seeds, threshold, min_samples)
        self._ck(self.L.glrtx_group_render_adaptive(self.h, C.byref(p), _fp(sd), sd.shape[0], C.byref(cfg)))
    def adaptive_active_tiles(self):
        """(active, total) tiles of the last selection, summed over the members (syncs)."""
        a, t = C.c_int(0), C.c_int(0)
        self._ck(self.L.glrtx_group_adaptive_active_tiles(self.h, C.byref(a), C.byref(t)))
        return int(a.value), int(t.value)
    def tile_mask(self):
        """Each member's last selection mask (its own owned-row tiles): a list of (tiles_y, tiles_x) uint8."""
        out = []
        for i in range(self.size()):
            m = self.L.glrtx_group_ctx(self.h, i)
            s = Stats()
            self.L.glrtx_get_stats(m, C.byref(s))
            out.append(np.zeros(((s.owned_rows + 7) // 8, (s.width + 7) // 8), np.uint8))
            rc = self.L.glrtx_read_tile_mask(m, out[-1].ctypes.data_as(C.POINTER(C.c_uint8)))
            if rc != 0:
                raise GlrtxError(rc, self.L.glrtx_last_error(m).decode())
        return out
    def read_adaptive_half(self):
        """Each member's half buffer: a list of (owned_rows, width, 4) float32."""
        return [_read_image(self.L, self.L.glrtx_group_ctx(self.h, i), self.L.glrtx_read_adaptive_half) for i in range(self.size())]

    def stats(self) -> Stats:
        s = Stats()
        self._ck(self.L.glrtx_group_get_stats(self.h, C.byref(s)))
        return s

    def read_accum(self) -> np.ndarray:
        out = np.zeros((self.hgt, self.w, 4), np.float32)
        self._ck(self.L.glrtx_group_read_accum(self.h, out.ctypes.data, self.w * 16))
        return out

    def gather_copies(self) -> int:
        return int(self.L.glrtx_group_gather_copies(self.h))

    def resolve_rgba8(self, gamma=2.2, flip_y=True) -> np.ndarray:
        out = np.zeros((self.hgt, self.w, 4), np.uint8)
        self._ck(self.L.glrtx_group_resolve_rgba8(self.h, out.ctypes.data, self.w * 4, gamma, int(flip_y)))
        return out

    def present_enable(self, ring, gamma=2.2, flip_y=True):
        """Every frame's image into a ring of `ring` pinned RGBA8 images (glrtx_group_present_enable: the FULL image); ring = 0 turns it off (untaken images are dropped)."""
        self._ck(self.L.glrtx_group_present_enable(self.h, int(ring), gamma, int(flip_y)))

    def present_acquire(self, wait=True):
        """The oldest image not yet acquired: a Presented (.frame, .rgba zero-copy view), or None when wait=False and it is not ready (GLRTX_EBUSY)."""
        img = Image()
        rc = self.L.glrtx_group_present_acquire(self.h, int(wait), C.byref(img))
        if rc == GLRTX_EBUSY and not wait:
            return None
        self._ck(rc)
        return Presented(img)

    def present_release(self, img):
        self._ck(self.L.glrtx_group_present_release(self.h, C.byref(img.img)))

    def present_stats(self) -> PresentStats:
        s = PresentStats()
        self._ck(self.L.glrtx_group_present_get_stats(self.h, C.byref(s)))
        return s


def render_image(scene, params, device_id=-1, count_rays=True):
    """Convenience: one pass from cleared accumulators on one GPU. Returns (accum (H,W,4), rays, kernel_ms)."""
    d = Device(device_id)
    try:
        d.upload_scene(scene)
        d.resize(params["width"], params["height"])
        d.count_rays(count_rays)
        d.render(params)
        d.sync()
        st = d.stats()
        return d.read_accum(), int(st.rays), float(st.kernel_ms_last)
    finally:
        d.close()
