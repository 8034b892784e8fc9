"""ctypes binding of libglrt_host.so (include/glrt_host.h): BVH builders and camera matrices.

CPU-only; loadable without a GPU.  Raises if the library has not been built
(`make -C opengl-raytracer_amd host` or `__graft_entry__.build()`).
"""
from __future__ import annotations

import ctypes as C
import pathlib

import numpy as np

PKG_ROOT = pathlib.Path(__file__).resolve().parents[2]
LIB_DIR = PKG_ROOT / "lib"

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = LIB_DIR / "libglrt_host.so"
        if not path.exists():
            raise RuntimeError(f"{path} is missing: run `make -C {PKG_ROOT}` (or __graft_entry__.build())")
        L = C.CDLL(str(path))
        fp = C.POINTER(C.c_float)
        L.glrt_bvh_node_count.restype = C.c_size_t
        L.glrt_bvh_node_count.argtypes = [C.c_size_t]
        L.glrt_bvh_build_sah.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.POINTER(C.c_int)]
        L.glrt_bvh_build_lbvh.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.POINTER(C.c_int)]
        L.glrt_bvh_build_sah_levels.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.POINTER(C.c_int)]
        L.glrt_bvh_build_chain.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp]
        L.glrt_bvh_build_reference.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.POINTER(C.c_int)]
        L.glrt_bvh_lights_first.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t]
        L.glrt_bvh_order_by_hits.argtypes = [fp, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]
        L.glrt_bvh_add_shadow_hits.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, fp, fp, C.c_size_t]
        L.glrt_bvh_reinsert.argtypes = [fp, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.glrt_bvh_refit.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t]
        L.glrt_trace_rays.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_int]
        L.glrt_render_features.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, fp] + [C.c_int] * 5 + [fp, fp]
        L.glrt_denoise_atrous.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, fp]
        L.glrt_fold_moments.argtypes = [fp, fp, C.c_int, C.c_int, C.c_int]
        L.glrt_variance_estimate.argtypes = [fp, fp, fp, fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, fp]
        L.glrt_denoise_variance.argtypes = [fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, fp, fp]
        L.glrt_adaptive_select_moments.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_uint8), fp]
        L.glrt_reproject.argtypes = [fp] * 9 + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.glrt_render_features_geom.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, fp] + [C.c_int] * 5 + [fp, fp, fp]
        L.glrt_reproject_motion.argtypes = [fp] * 6 + [C.c_size_t, fp, C.c_size_t, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, fp,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.glrt_reproject_moments.argtypes = [fp] * 10 + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.glrt_reproject_motion_moments.argtypes = [fp] * 7 + [C.c_size_t, fp, C.c_size_t, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, fp, fp,
                                                    C.POINTER(C.c_int), C.POINTER(C.c_int)]
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.glrt_exposure_measure.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, fp, u32p, u64p, u64p, fp, fp, fp]
        L.glrt_tonemap.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, fp, C.POINTER(C.c_uint8)]
        L.glrt_bloom.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, fp, fp]
        L.glrt_fold_cascades.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float]
        L.glrt_reweight.argtypes = [fp, C.c_int, C.c_int, C.c_float, fp]
        L.glrt_skin_vertices.argtypes = [fp, C.c_size_t, C.POINTER(C.c_int32), fp, fp, C.c_int, fp]
        L.glrt_deform_vertices.argtypes = [fp, C.c_size_t, C.POINTER(C.c_int32), fp, fp, C.c_int, C.c_int, fp, fp, C.c_int, fp]
        L.glrt_deform_vertices_sparse.argtypes = [fp, C.c_size_t, C.POINTER(C.c_int32), fp, fp, C.c_int, C.c_int, u64p, u32p, fp, fp, C.c_int, fp]
        L.glrt_morph_sparsify.argtypes = [fp, C.c_int, C.c_size_t, u64p, u32p, fp]
        L.glrt_dualquat_from_matrix.argtypes = [fp, fp]
        u8p = C.POINTER(C.c_uint8)
        L.glrt_normal_topology.argtypes = [fp, C.c_size_t, fp, C.c_size_t, C.c_uint, u32p, u8p, C.POINTER(C.c_size_t)]
        L.glrt_rebuild_normals.argtypes = [fp, C.c_size_t, fp, C.c_size_t, u32p, u8p]
        L.glrt_positions_to_vertices.argtypes = [fp, fp, C.c_size_t, fp]
        L.glrt_dualquat_from_matrix.restype = None
        i32p = C.POINTER(C.c_int32)
        L.glrt_texture_lookup.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, i32p, fp, C.c_size_t, fp]
        L.glrt_srgb_table.restype = fp
        L.glrt_srgb_table.argtypes = []
        L.glrt_texture_albedo.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, i32p, fp, C.c_size_t, fp]
        L.glrt_texture_channel.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, i32p, i32p, fp, C.c_size_t, fp]
        L.glrt_render_features_geom_cutout.argtypes = ([fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, fp] + [C.c_int] * 5 +
                                                       [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, i32p, C.c_void_p, fp, fp, fp])
        L.glrt_light_st.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp]
        L.glrt_light_emission.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, i32p, i32p, fp, C.c_size_t, fp]
        L.glrt_emission_albedo.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, i32p, i32p, fp, C.c_size_t, fp]
        L.glrt_emission_bind_check.argtypes = [fp, C.c_size_t, C.c_size_t, C.c_int, i32p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.glrt_launch_route.argtypes = [C.POINTER(RouteState), C.c_int, C.POINTER(Route), C.c_char_p, C.c_size_t]
        L.glrt_surface_create.argtypes = [fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, i32p, C.c_void_p,
                                          i32p, C.POINTER(C.c_void_p)]
        L.glrt_surface_free.restype = None
        L.glrt_surface_free.argtypes = [C.c_void_p]
        L.glrt_surface_albedo.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, fp]
        L.glrt_surface_accept.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
        L.glrt_surface_emission.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, fp]
        vp = C.c_void_p
        L.glrt_env_weights.argtypes = [vp, vp, C.c_size_t, vp, fp, i32p]
        L.glrt_env_alias.argtypes = [fp, C.c_int32, fp, i32p, fp, i32p, fp]
        L.glrt_env_sample.argtypes = [vp, vp, C.c_size_t, vp, fp, C.c_size_t, fp]
        L.glrt_env_eval.argtypes = [vp, vp, C.c_size_t, vp, fp, C.c_size_t, fp]
        L.glrt_env_from_latlong.argtypes = [fp, C.c_int32, C.c_int32, C.c_int32, fp]
        L.glrt_map_decode.argtypes = [fp, C.c_size_t, fp]
        L.glrt_map_normal.argtypes = [fp, C.c_size_t, C.c_float, fp]
        L.glrt_map_alpha.argtypes = [fp, C.c_size_t, fp]
        L.glrt_look_at.argtypes = [fp, fp, fp, fp]
        L.glrt_perspective.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, fp]
        L.glrt_mat4_mul.argtypes = [fp, fp, fp]
        L.glrt_mat4_inverse.argtypes = [fp, fp]
        L.glrt_frame_seed.argtypes = [C.c_uint32, fp]
        _lib = L
    return _lib


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def build_bvh(vert: np.ndarray, tri: np.ndarray, kind: str = "sah"):
    """vert: (nV*5, 3) float32 texels, tri: (nT, 4).  Returns (nodes (nN*3, 3) float32, max_depth)."""
    L = lib()
    vert = _f32(vert).reshape(-1, 15)
    tri = _f32(tri).reshape(-1, 4)
    n = int(L.glrt_bvh_node_count(tri.shape[0]))
    nodes = np.zeros((n * 3, 3), np.float32)
    depth = C.c_int(0)
    if kind == "sah-reinsert":  # "sah" + the insertion-based optimisation pass (as glrt::Scene::parse's builder of that name)
        nodes, depth = build_bvh(vert, tri, "sah")
        out, d2, _, _ = reinsert(nodes)
        return out, (d2 if d2 >= 0 else depth)
    if kind == "sah":
        rc = L.glrt_bvh_build_sah(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), C.byref(depth))
    elif kind == "lbvh":
        rc = L.glrt_bvh_build_lbvh(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), C.byref(depth))
    elif kind == "sahl":  # binned SAH by levels + exact sweep at the bottom: the CPU statement of the device builder glrtx_build_bvh_sah
        rc = L.glrt_bvh_build_sah_levels(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), C.byref(depth))
    elif kind == "reference":  # the reference host's own tree, restated rule for rule (bvh.cpp:72-160); never re-ordered afterwards
        rc = L.glrt_bvh_build_reference(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), C.byref(depth))
    elif kind == "chain":
        rc = L.glrt_bvh_build_chain(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes))
        depth.value = 2
    else:
        raise ValueError(kind)
    if rc != 0:
        raise RuntimeError(f"glrt_bvh_build_{kind} failed: {rc}")
    return nodes, depth.value


def lights_first(nodes, tri, mat):
    """glrt_bvh_lights_first on a copy of `nodes`: the child whose subtree holds the emitting triangles into the slot the traversal visits first, at every fork where
    only one child has any.  Returns (nodes (nN*3, 3) float32, forks exchanged).  GLRT_BVH_LIGHTS_FIRST=0 in the environment returns the tree unchanged."""
    import os
    out = _f32(nodes).reshape(-1, 3).copy()
    if os.environ.get("GLRT_BVH_LIGHTS_FIRST", "1") == "0":
        return out, 0
    tri, mat = _f32(tri).reshape(-1, 4), _f32(mat).reshape(-1, 18)
    rc = lib().glrt_bvh_lights_first(_fp(out), out.shape[0] // 3, _fp(tri), tri.shape[0], _fp(mat), mat.shape[0])
    if rc < 0:
        raise RuntimeError(f"glrt_bvh_lights_first failed: {rc}")
    return out, int(rc)


def order_by_hits(nodes, tri_hits, tri=None, mat=None):
    """glrt_bvh_order_by_hits on a copy of `nodes`: at every fork the child whose subtree collected more closest hits in a calibration frame (device.Device.hit_histogram)
    into the slot the traversal visits first.  With `tri` and `mat` the shadow rays' share is added first (glrt_bvh_add_shadow_hits).  Returns (nodes, forks exchanged)."""
    out = _f32(nodes).reshape(-1, 3).copy()
    h = np.ascontiguousarray(tri_hits, dtype=np.uint32).copy()
    if tri is not None and mat is not None:
        t, m = _f32(tri).reshape(-1, 4), _f32(mat).reshape(-1, 18)
        rc = lib().glrt_bvh_add_shadow_hits(h.ctypes.data_as(C.POINTER(C.c_uint32)), h.shape[0], _fp(t), _fp(m), m.shape[0])
        if rc < 0:
            raise RuntimeError(f"glrt_bvh_add_shadow_hits failed: {rc}")
    rc = lib().glrt_bvh_order_by_hits(_fp(out), out.shape[0] // 3, h.ctypes.data_as(C.POINTER(C.c_uint32)), h.shape[0])
    if rc < 0:
        raise RuntimeError(f"glrt_bvh_order_by_hits failed: {rc}")
    return out, int(rc)


def reinsert(nodes, max_passes: int = 8):
    """glrt_bvh_reinsert on a copy of `nodes`: insertion-based optimisation of a finished tree.  Returns (nodes (nN*3, 3) float32, max depth (-1: left alone),
    subtrees moved, (cost before, cost after)) -- cost = summed area of the forks' boxes / the root's."""
    out = _f32(nodes).reshape(-1, 3).copy()
    depth = C.c_int(0)
    cost = (C.c_double * 2)()
    rc = lib().glrt_bvh_reinsert(_fp(out), out.shape[0] // 3, int(max_passes), C.byref(depth), cost)
    if rc == -3:  # GLRT_HOST_EDEPTH: the optimised tree would be deeper than the traversal stack allows; `out` is the input tree again
        return out, -1, 0, (cost[0], cost[1])
    if rc < 0:
        raise RuntimeError(f"glrt_bvh_reinsert failed: {rc}")
    return out, depth.value, int(rc), (cost[0], cost[1])


def refit_bvh(vert, tri, nodes):
    """glrt_bvh_refit on a copy of `nodes`: the boxes of the tree's reachable nodes recomputed from `vert` (leaves from their triangle's positions, forks from their
    children, in the total order on float bit patterns of include/glrt_host.h); topology untouched.  Returns nodes (nN*3, 3) float32."""
    vert, tri = _f32(vert).reshape(-1, 15), _f32(tri).reshape(-1, 4)
    out = _f32(nodes).reshape(-1, 3).copy()
    rc = lib().glrt_bvh_refit(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(out), out.shape[0] // 3)
    if rc != 0:
        raise RuntimeError(f"glrt_bvh_refit failed: {rc}")
    return out


TRACE_CLOSEST, TRACE_ANY = 0, 1  # glrt_trace_rays / glrtx_trace_rays flags


def trace_rays(vert, tri, nodes, rays, any_hit=False):
    """glrt_trace_rays: the CPU statement of the device's ray queries on a wire-format tree (include/glrt_host.h).  rays: (n, 8) float32
    {ox, oy, oz, tmin, dx, dy, dz, tmax}.  Returns (t, tri, u, v): views of one (n, 4) buffer, tri as int32 (the wire triangle index, -1 on a miss)."""
    vert, tri = _f32(vert).reshape(-1, 15), _f32(tri).reshape(-1, 4)
    nodes = _f32(nodes).reshape(-1, 9)
    r = _f32(rays).reshape(-1, 8)
    out = np.zeros((r.shape[0], 4), np.float32)
    rc = lib().glrt_trace_rays(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), nodes.shape[0], _fp(r), r.shape[0], _fp(out),
                               TRACE_ANY if any_hit else TRACE_CLOSEST)
    if rc != 0:
        raise RuntimeError(f"glrt_trace_rays failed: {rc}")
    return out[:, 0], out[:, 1].view(np.int32), out[:, 2], out[:, 3]


def render_features(scene, params, width=None, height=None, rank=0, world=1, stripe=16):
    """glrt_render_features: the CPU statement of Device.render_features (include/glrt_host.h) for the rows a partition owns (default: the whole image).
    Returns (normal_depth, albedo_id): (owned_rows, width, 4) float32 each; albedo_id[..., 3] holds the material id as int32 bits (-1: a miss)."""
    w, h = int(width or params["width"]), int(height or params["height"])
    vert, tri = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["tri"]).reshape(-1, 4)
    nodes, mat = _f32(scene["bvh"]).reshape(-1, 9), _f32(scene["mat"]).reshape(-1, 18)
    c2w, s2c = _f32(params["c2w"]).reshape(16), _f32(params["s2c"]).reshape(16)
    rows = sum(1 for y in range(h) if (y // stripe) % world == rank)
    n, a = np.zeros((rows, w, 4), np.float32), np.zeros((rows, w, 4), np.float32)
    rc = lib().glrt_render_features(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), nodes.shape[0], _fp(mat), mat.shape[0], _fp(c2w), _fp(s2c),
                                    w, h, rank, world, stripe, _fp(n), _fp(a))
    if rc != 0:
        raise RuntimeError(f"glrt_render_features failed: {rc}")
    return n, a


def render_features_geom(scene, params, width=None, height=None, rank=0, world=1, stripe=16):
    """glrt_render_features_geom: render_features with the geometry plane, the CPU statement of the feature pass under Device.track_motion.  Returns
    (normal_depth, albedo_id, geom); geom[..., 0] holds the wire triangle index as int32 bits (-1: a miss), geom[..., 1:3] the hit's barycentrics."""
    w, h = int(width or params["width"]), int(height or params["height"])
    vert, tri = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["tri"]).reshape(-1, 4)
    nodes, mat = _f32(scene["bvh"]).reshape(-1, 9), _f32(scene["mat"]).reshape(-1, 18)
    c2w, s2c = _f32(params["c2w"]).reshape(16), _f32(params["s2c"]).reshape(16)
    rows = sum(1 for y in range(h) if (y // stripe) % world == rank)
    n, a, g = (np.zeros((rows, w, 4), np.float32) for _ in range(3))
    rc = lib().glrt_render_features_geom(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), nodes.shape[0], _fp(mat), mat.shape[0], _fp(c2w), _fp(s2c),
                                         w, h, rank, world, stripe, _fp(n), _fp(a), _fp(g))
    if rc != 0:
        raise RuntimeError(f"glrt_render_features_geom failed: {rc}")
    return n, a, g


# The denoiser's defaults (DESIGN.md "Denoising": chosen from the sweep recorded there); Device.denoise takes the same.
DENOISE_DEFAULTS = dict(iterations=5, sigma_color=100.0, sigma_normal=0.1, sigma_depth=0.01, demodulate=True)


def denoise_atrous(accum, normal_depth, albedo_id, iterations=DENOISE_DEFAULTS["iterations"], sigma_color=DENOISE_DEFAULTS["sigma_color"],
                   sigma_normal=DENOISE_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"], demodulate=DENOISE_DEFAULTS["demodulate"]):
    """glrt_denoise_atrous: the CPU statement of Device.denoise on (rows, width, 4) float32 arrays.  Returns D, float4(rgb, 1) per pixel."""
    a, n, al = _f32(accum), _f32(normal_depth), _f32(albedo_id)
    if a.ndim != 3 or a.shape[2] != 4 or n.shape != a.shape or al.shape != a.shape:
        raise ValueError(f"denoise_atrous: three (rows, width, 4) arrays of one shape expected, got {a.shape}, {n.shape}, {al.shape}")
    out = np.zeros_like(a)
    rc = lib().glrt_denoise_atrous(_fp(a), _fp(n), _fp(al), a.shape[1], a.shape[0], int(iterations), float(sigma_color), float(sigma_normal),
                                   float(sigma_depth), int(bool(demodulate)), _fp(out))
    if rc != 0:
        raise RuntimeError(f"glrt_denoise_atrous failed: {rc}")
    return out


# The variance-guided filter's defaults (DESIGN.md "Variance guidance": chosen from the sweep recorded there); Device.denoise_variance takes the same.
DENOISE_VAR_DEFAULTS = dict(iterations=5, sigma_lum=4.0, sigma_normal=0.1, sigma_depth=0.01, demodulate=True)


def _four_planes(name, *arrs):
    arr = [_f32(v) for v in arrs]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"{name}: (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    return arr


def fold_moments(moments, planes):
    """glrt_fold_moments: the sample planes (k, rows, width, 4), in order, folded into a copy of the moments plane M {sum l, sum l^2, 0, count}."""
    m = _f32(moments).copy()
    p = _f32(planes)
    if m.ndim != 3 or m.shape[2] != 4 or p.ndim != 4 or p.shape[1:] != m.shape:
        raise ValueError(f"fold_moments: moments (rows, width, 4) and planes (k, rows, width, 4) expected, got {m.shape} and {p.shape}")
    rc = lib().glrt_fold_moments(_fp(m), _fp(p), p.shape[0], m.shape[1], m.shape[0])
    if rc != 0:
        raise RuntimeError(f"glrt_fold_moments failed: {rc}")
    return m


def variance_estimate(accum, moments, normal_depth, albedo_id, sigma_normal=DENOISE_VAR_DEFAULTS["sigma_normal"],
                      sigma_depth=DENOISE_VAR_DEFAULTS["sigma_depth"], demodulate=DENOISE_VAR_DEFAULTS["demodulate"]):
    """glrt_variance_estimate: the CPU statement of the variance pass.  Returns V0, (rows, width) float32."""
    a, m, n, al = _four_planes("variance_estimate", accum, moments, normal_depth, albedo_id)
    v0 = np.zeros(a.shape[:2], np.float32)
    rc = lib().glrt_variance_estimate(_fp(a), _fp(m), _fp(n), _fp(al), a.shape[1], a.shape[0], float(sigma_normal), float(sigma_depth), int(bool(demodulate)), _fp(v0))
    if rc != 0:
        raise RuntimeError(f"glrt_variance_estimate failed: {rc}")
    return v0


def adaptive_select_moments(moments, threshold, min_samples):
    """glrt_adaptive_select_moments: the CPU statement of Device.render_adaptive_moments' selection on a moments plane (rows, width, 4) float32.
    Returns (mask (tiles_y, tiles_x) uint8, E (tiles_y, tiles_x) float32, a NaN as 0x7FC00000)."""
    m = _f32(moments)
    if m.ndim != 3 or m.shape[2] != 4:
        raise ValueError(f"adaptive_select_moments: moments must be (rows, width, 4), got {m.shape}")
    rows, width = m.shape[:2]
    mask = np.zeros(((rows + 7) // 8, (width + 7) // 8), np.uint8)
    err = np.zeros(mask.shape, np.float32)
    rc = lib().glrt_adaptive_select_moments(_fp(m), width, rows, float(threshold), int(min_samples), mask.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(err))
    if rc != 0:
        raise RuntimeError(f"glrt_adaptive_select_moments failed: {rc}")
    return mask, err


def denoise_variance(accum, moments, normal_depth, albedo_id, iterations=DENOISE_VAR_DEFAULTS["iterations"], sigma_lum=DENOISE_VAR_DEFAULTS["sigma_lum"],
                     sigma_normal=DENOISE_VAR_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_VAR_DEFAULTS["sigma_depth"],
                     demodulate=DENOISE_VAR_DEFAULTS["demodulate"], return_v0=False):
    """glrt_denoise_variance: the CPU statement of Device.denoise_variance on (rows, width, 4) float32 arrays.  Returns D, float4(rgb, 1) per pixel (with
    return_v0: (D, V0))."""
    a, m, n, al = _four_planes("denoise_variance", accum, moments, normal_depth, albedo_id)
    out = np.zeros_like(a)
    v0 = np.zeros(a.shape[:2], np.float32) if return_v0 else None
    rc = lib().glrt_denoise_variance(_fp(a), _fp(m), _fp(n), _fp(al), a.shape[1], a.shape[0], int(iterations), float(sigma_lum), float(sigma_normal),
                                     float(sigma_depth), int(bool(demodulate)), _fp(out), _fp(v0) if return_v0 else None)
    if rc != 0:
        raise RuntimeError(f"glrt_denoise_variance failed: {rc}")
    return (out, v0) if return_v0 else out


# The reprojection's defaults (DESIGN.md "Reprojection": chosen from the sweep recorded there); Device.reproject takes the same.
# glrtx_tonemap_cfg's defaults (include/glrtx.h "Tone mapping") and the names of its ops
TONEMAP_DEFAULTS = dict(op=0, source=0, auto_exposure=0, exposure=1.0, key=0.18, low_permille=500, high_permille=950, adapt=1.0, white=4.0, gamma=2.2, flip_y=1)
TONEMAP_OPS = dict(clamp=0, reinhard=1, aces=2)


def exposure_measure(src, exposure_in=None, key=TONEMAP_DEFAULTS["key"], low_permille=TONEMAP_DEFAULTS["low_permille"],
                     high_permille=TONEMAP_DEFAULTS["high_permille"], adapt=TONEMAP_DEFAULTS["adapt"]):
    """glrt_exposure_measure: the CPU statement of one exposure measurement on a (rows, width, 4) float32 array; exposure_in: the previous E, None for a first
    measurement.  Returns a dict: hist (256 uint32), counted, kept, mean_log2, target, exposure (float32)."""
    a = _f32(src)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"exposure_measure: a (rows, width, 4) array expected, got {a.shape}")
    hist = np.zeros(256, np.uint32)
    n, k = C.c_uint64(0), C.c_uint64(0)
    f = np.zeros(3, np.float32)
    prev = None if exposure_in is None else np.array([exposure_in], np.float32)
    rc = lib().glrt_exposure_measure(_fp(a), a.shape[1], a.shape[0], float(key), int(low_permille), int(high_permille), float(adapt),
                                     None if prev is None else _fp(prev), hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n), C.byref(k),
                                     _fp(f[0:1]), _fp(f[1:2]), _fp(f[2:3]))
    if rc != 0:
        raise RuntimeError(f"glrt_exposure_measure failed: {rc}")
    return dict(hist=hist, counted=int(n.value), kept=int(k.value), mean_log2=f[0], target=f[1], exposure=f[2])


def tonemap(src, op=TONEMAP_DEFAULTS["op"], auto_exposure=TONEMAP_DEFAULTS["auto_exposure"], exposure=TONEMAP_DEFAULTS["exposure"], E=1.0,
            white=TONEMAP_DEFAULTS["white"], gamma=TONEMAP_DEFAULTS["gamma"], flip_y=TONEMAP_DEFAULTS["flip_y"]):
    """glrt_tonemap: the CPU statement of the tone curve and of the resolve behind it on a (rows, width, 4) float32 array; E: the measured exposure (read when
    auto_exposure).  Returns (T (rows, width, 4) float32 {y, 1}, bytes (rows, width, 4) uint8)."""
    a = _f32(src)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"tonemap: a (rows, width, 4) array expected, got {a.shape}")
    t, b = np.zeros_like(a), np.zeros(a.shape, np.uint8)
    rc = lib().glrt_tonemap(_fp(a), a.shape[1], a.shape[0], TONEMAP_OPS.get(op, op) if isinstance(op, str) else int(op), int(bool(auto_exposure)), float(exposure),
                            float(E), float(white), float(gamma), int(bool(flip_y)), _fp(t), b.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise RuntimeError(f"glrt_tonemap failed: {rc}")
    return t, b


# glrtx_bloom_cfg's defaults (include/glrtx.h "Bloom": conventional values, not tuned on anything)
BLOOM_DEFAULTS = dict(source=0, threshold=1.0, strength=0.25, levels=5)


def bloom_texels(width, rows, levels):
    """The number of texels in the packed pyramid D_1 .. D_levels of a width x rows image: w_{k+1} = (w_k + 1) >> 1."""
    n, w, h = 0, int(width), int(rows)
    for _ in range(int(levels)):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        n += w * h
    return n


def bloom(src, threshold=BLOOM_DEFAULTS["threshold"], strength=BLOOM_DEFAULTS["strength"], levels=BLOOM_DEFAULTS["levels"]):
    """glrt_bloom: the CPU statement of the bloom pass on a (rows, width, 4) float32 array.  Returns (d, B): d the planes D_1 .. D_levels packed back to back,
    (n, 4) float32 with w = 0; B (rows, width, 4) float32 {x + strength * glow, 1}."""
    a = _f32(src)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"bloom: a (rows, width, 4) array expected, got {a.shape}")
    if not 1 <= int(levels) <= 8:
        raise RuntimeError(f"glrt_bloom failed: levels {levels} outside 1..8")
    d, b = np.zeros((bloom_texels(a.shape[1], a.shape[0], levels), 4), np.float32), np.zeros_like(a)
    rc = lib().glrt_bloom(_fp(a), a.shape[1], a.shape[0], float(threshold), float(strength), int(levels), _fp(d), _fp(b))
    if rc != 0:
        raise RuntimeError(f"glrt_bloom failed: {rc}")
    return d, b


REWEIGHT_DEFAULTS = dict(kappa=4.0, start=1.0)


def fold_cascades(cascades, planes, accum=None, start=REWEIGHT_DEFAULTS["start"]):
    """glrt_fold_cascades: the sample planes (k, rows, width, 4), in order, folded into a copy of the cascade planes C (6, rows, width, 4) {sum w rgb, count}
    (None: zeros) and, with `accum` (rows, width, 4), into a copy of that accumulator as the device's pass does.  Returns C, or (C, accumulator) with `accum`."""
    p = _f32(planes)
    if p.ndim != 4 or p.shape[3] != 4:
        raise ValueError(f"fold_cascades: planes (k, rows, width, 4) expected, got {p.shape}")
    c = np.zeros((6,) + p.shape[1:], np.float32) if cascades is None else _f32(cascades).copy()
    if c.shape != (6,) + p.shape[1:]:
        raise ValueError(f"fold_cascades: cascades (6, rows, width, 4) matching the planes expected, got {c.shape} and {p.shape}")
    a = None if accum is None else _f32(accum).copy()
    if a is not None and a.shape != p.shape[1:]:
        raise ValueError(f"fold_cascades: accum (rows, width, 4) matching the planes expected, got {a.shape}")
    rc = lib().glrt_fold_cascades(_fp(c), None if a is None else _fp(a), _fp(p), p.shape[0], p.shape[2], p.shape[1], float(start))
    if rc != 0:
        raise RuntimeError(f"glrt_fold_cascades failed: {rc}")
    return c if a is None else (c, a)


def reweight(cascades, kappa=REWEIGHT_DEFAULTS["kappa"]):
    """glrt_reweight: the CPU statement of Device.reweight on cascade planes (6, rows, width, 4).  Returns D (rows, width, 4) float32 {rgb, 1}."""
    c = _f32(cascades)
    if c.ndim != 4 or c.shape[0] != 6 or c.shape[3] != 4:
        raise ValueError(f"reweight: cascades must be (6, rows, width, 4), got {c.shape}")
    out = np.empty(c.shape[1:], np.float32)
    rc = lib().glrt_reweight(_fp(c), c.shape[2], c.shape[1], float(kappa), _fp(out))
    if rc != 0:
        raise RuntimeError(f"glrt_reweight failed: {rc}")
    return out


def rig_arrays(name, rest, bones, weights, matrices=None):
    """The arrays of a rig as the C calls take them: rest (n, 15) float32, bones (n, 4) int32, weights (n, 4) float32 and, if given, matrices (n_bones, 12)
    float32 (also accepted as (n_bones, 3, 4)).  Bits are kept: float32 input is not converted."""
    r = _f32(rest).reshape(-1, 15)
    b = np.ascontiguousarray(bones, dtype=np.int32).reshape(-1, 4)
    w = _f32(weights).reshape(-1, 4)
    if not (r.shape[0] == b.shape[0] == w.shape[0]):
        raise ValueError(f"{name}: {r.shape[0]} vertices, {b.shape[0]} bone records, {w.shape[0]} weight records")
    if matrices is None:
        return r, b, w
    m = _f32(matrices)
    if m.size % 12 or m.size == 0:
        raise ValueError(f"{name}: matrices must be (n_bones, 12) or (n_bones, 3, 4), got {m.shape}")
    return r, b, w, m.reshape(-1, 12)


def skin_vertices(rest, bones, weights, matrices):
    """glrt_skin_vertices: the CPU statement of Device.pose / device.debug_skin (include/glrtx.h "Posing").  Returns the posed vertices (n, 15) float32."""
    r, b, w, m = rig_arrays("skin_vertices", rest, bones, weights, matrices)
    out = np.zeros_like(r)
    rc = lib().glrt_skin_vertices(_fp(r), r.shape[0], b.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), _fp(m), m.shape[0], _fp(out))
    if rc != 0:
        raise RuntimeError(f"glrt_skin_vertices failed: {rc}")
    return out


def deform_arrays(name, rest, bones, weights, bone_data, mode, deltas, morph_weights):
    """rig_arrays plus the bone data of `mode` -- (n_bones, 12) matrices or (n_bones, 8) dual quaternions --, the deltas (n_targets, n, 6) and the morph weights
    (n_targets,), both empty when there are no targets.  Bits are kept."""
    r, b, w = rig_arrays(name, rest, bones, weights)
    per = 8 if mode else 12
    m = _f32(bone_data)
    if m.size % per or m.size == 0:
        raise ValueError(f"{name}: mode {mode} takes (n_bones, {per}) bone data, got {m.shape}")
    mw = np.zeros(0, np.float32) if morph_weights is None else _f32(morph_weights).reshape(-1)
    d = np.zeros((0, r.shape[0], 6), np.float32) if deltas is None else _f32(deltas)
    if d.shape != (mw.size, r.shape[0], 6):
        raise ValueError(f"{name}: deltas {d.shape}, expected ({mw.size}, {r.shape[0]}, 6) for {mw.size} morph weights")
    return r, b, w, m.reshape(-1, per), d, mw


def deform_vertices(rest, bones, weights, bone_data, mode=0, deltas=None, morph_weights=None):
    """glrt_deform_vertices: the CPU statement of Device.pose_morph / Device.pose_dualquat / device.debug_deform (include/glrtx.h "Deforming").  mode 0: bone_data
    is (n_bones, 12) matrices; mode 1: (n_bones, 8) dual quaternions.  Returns the deformed vertices (n, 15) float32."""
    r, b, w, m, d, mw = deform_arrays("deform_vertices", rest, bones, weights, bone_data, mode, deltas, morph_weights)
    out = np.zeros_like(r)
    rc = lib().glrt_deform_vertices(_fp(r), r.shape[0], b.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), _fp(m), m.shape[0], int(mode),
                                    _fp(d) if mw.size else None, _fp(mw) if mw.size else None, mw.size, _fp(out))
    if rc != 0:
        raise RuntimeError(f"glrt_deform_vertices failed: {rc}")
    return out


def sparse_arrays(name, offsets, vertex, deltas):
    """A sparse morph-target set as the C calls take it: offsets (n_targets + 1,) uint64, vertex (nnz,) uint32, deltas (nnz, 6) float32; None for all three is
    the set of no targets.  Only the shapes are looked at here: what the set holds is the library's to check.  Bits are kept."""
    if offsets is None:
        return np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 6), np.float32)
    o = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    v = np.zeros(0, np.uint32) if vertex is None else np.ascontiguousarray(vertex, dtype=np.uint32).reshape(-1)
    d = np.zeros((0, 6), np.float32) if deltas is None else _f32(deltas).reshape(-1, 6)
    if o.size < 1 or v.size != d.shape[0]:
        raise ValueError(f"{name}: {o.size} offsets, {v.size} vertex indices, {d.shape[0]} delta records")
    return o, v, d


def sparse_pointers(o, v, d):
    """The three ctypes pointers of sparse_arrays' result; an empty vertex or deltas array goes in as NULL."""
    return (o.ctypes.data_as(C.POINTER(C.c_uint64)), v.ctypes.data_as(C.POINTER(C.c_uint32)) if v.size else None, _fp(d) if d.size else None)


def deform_vertices_sparse(rest, bones, weights, bone_data, mode=0, offsets=None, vertex=None, deltas=None, morph_weights=None):
    """glrt_deform_vertices_sparse: the CPU statement of Device.pose_morph / Device.pose_dualquat on a rig with a sparse set and of device.debug_deform_sparse
    (include/glrtx.h "Deforming", SPARSE TARGETS).  offsets (n_targets + 1,), vertex (nnz,), deltas (nnz, 6), morph_weights (n_targets,).  Returns (n, 15)."""
    r, b, w, m, _, _ = deform_arrays("deform_vertices_sparse", rest, bones, weights, bone_data, mode, None, None)
    o, v, d = sparse_arrays("deform_vertices_sparse", offsets, vertex, deltas)
    mw = np.zeros(0, np.float32) if morph_weights is None else _f32(morph_weights).reshape(-1)
    if mw.size != o.size - 1:
        raise ValueError(f"deform_vertices_sparse: {mw.size} morph weights for {o.size - 1} targets")
    out = np.zeros_like(r)
    po, pv, pd = sparse_pointers(o, v, d)
    rc = lib().glrt_deform_vertices_sparse(_fp(r), r.shape[0], b.ctypes.data_as(C.POINTER(C.c_int32)), _fp(w), _fp(m), m.shape[0], int(mode), po, pv, pd,
                                           _fp(mw) if mw.size else None, mw.size, _fp(out))
    if rc != 0:
        raise RuntimeError(f"glrt_deform_vertices_sparse failed: {rc}")
    return out


def morph_sparsify(deltas):
    """glrt_morph_sparsify: dense deltas (n_targets, n_vert, 6) float32 -> (offsets (n_targets + 1,) uint64, vertex (nnz,) uint32, deltas (nnz, 6) float32), the
    entries with a component whose exponent field is not 0.  The counting call first, then the filling call."""
    d = _f32(deltas)
    if d.ndim != 3 or d.shape[2] != 6:
        raise ValueError(f"morph_sparsify: deltas must be (n_targets, n_vert, 6), got {d.shape}")
    L = lib()
    o = np.zeros(d.shape[0] + 1, np.uint64)
    po = o.ctypes.data_as(C.POINTER(C.c_uint64))
    src = _fp(d) if d.size else None
    rc = L.glrt_morph_sparsify(src, d.shape[0], d.shape[1], po, None, None)
    if rc != 0:
        raise RuntimeError(f"glrt_morph_sparsify failed: {rc}")
    nnz = int(o[-1])
    v, out = np.zeros(nnz, np.uint32), np.zeros((nnz, 6), np.float32)
    if nnz:
        rc = L.glrt_morph_sparsify(src, d.shape[0], d.shape[1], po, v.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(out))
        if rc != 0 or int(o[-1]) != nnz:
            raise RuntimeError(f"glrt_morph_sparsify failed: {rc} ({int(o[-1])} entries after {nnz} counted)")
    return o, v, out


def dualquat_from_matrix(m):
    """glrt_dualquat_from_matrix: the eight floats {r.xyzw, d.xyzw} of one rigid 3x4 matrix (12 floats, row-major)."""
    a = _f32(m).reshape(12)
    out = np.zeros(8, np.float32)
    lib().glrt_dualquat_from_matrix(_fp(a), _fp(out))
    return out


NORMALS_WELD_POSITIONS = 1  # GLRT_NORMALS_WELD_POSITIONS
NORMAL_CHUNK = 256  # GLRT_NORMAL_CHUNK


def normals_arrays(name, vert, tri, class_of_vertex=None, flip=None):
    """The arrays of a normal rebuild as the C calls take them: vert (n, 15) float32, tri (n_tri, 4) float32 and, if given, the class map (n,) uint32 and the
    flip bytes (n_tri,) uint8.  Only the shapes are looked at here.  Bits are kept: float32 input is not converted."""
    v = _f32(vert).reshape(-1, 15)
    t = _f32(tri).reshape(-1, 4)
    if class_of_vertex is None:
        return v, t
    c = np.ascontiguousarray(class_of_vertex, dtype=np.uint32).reshape(-1)
    f = np.ascontiguousarray(flip, dtype=np.uint8).reshape(-1)
    if c.size != v.shape[0] or f.size != t.shape[0]:
        raise ValueError(f"{name}: {v.shape[0]} vertices with {c.size} class ids, {t.shape[0]} triangles with {f.size} flip bytes")
    return v, t, c, f


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a.size else None


def normal_topology(rest, tri, flags=0):
    """glrt_normal_topology (include/glrtx.h "Rebuilding normals", TOPOLOGY): the weld classes of the rest vertices (n, 15) and the orientation of the wire
    triangles (n_tri, 4).  Returns (class_of_vertex (n,) uint32, flip (n_tri,) uint8, n_classes)."""
    v, t = normals_arrays("normal_topology", rest, tri)
    c, f, n = np.zeros(v.shape[0], np.uint32), np.zeros(t.shape[0], np.uint8), C.c_size_t(0)
    rc = lib().glrt_normal_topology(_ptr(v, C.c_float), v.shape[0], _ptr(t, C.c_float), t.shape[0], int(flags), _ptr(c, C.c_uint32), _ptr(f, C.c_uint8), C.byref(n))
    if rc != 0:
        raise RuntimeError(f"glrt_normal_topology failed: {rc}")
    return c, f, int(n.value)


def rebuild_normals(vert, tri, class_of_vertex, flip):
    """glrt_rebuild_normals: the CPU statement of Device.update_positions, of a pose under Device.set_pose_normals and of device.debug_rebuild_normals
    (include/glrtx.h "Rebuilding normals", REBUILD).  Returns a copy of vert (n, 15) float32 with its normal words rebuilt from its position words."""
    v, t, c, f = normals_arrays("rebuild_normals", vert, tri, class_of_vertex, flip)
    out = v.copy()
    rc = lib().glrt_rebuild_normals(_ptr(out, C.c_float), out.shape[0], _ptr(t, C.c_float), t.shape[0], _ptr(c, C.c_uint32), _ptr(f, C.c_uint8))
    if rc != 0:
        raise RuntimeError(f"glrt_rebuild_normals failed: {rc}")
    return out


def positions_to_vertices(rest, pos):
    """glrt_positions_to_vertices: the rest records (n, 15) with their position words replaced by pos (n, 3), moved as integers."""
    r = _f32(rest).reshape(-1, 15)
    p = _f32(pos).reshape(-1, 3)
    if p.shape[0] != r.shape[0]:
        raise ValueError(f"positions_to_vertices: {r.shape[0]} vertices, {p.shape[0]} positions")
    out = np.zeros_like(r)
    rc = lib().glrt_positions_to_vertices(_ptr(r, C.c_float), _ptr(p, C.c_float), r.shape[0], _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_positions_to_vertices failed: {rc}")
    return out


# Textures (include/glrtx.h "Textures"): GLRT_TEX_* / GLRTX_TEX_*
TEX_RGBA32F, TEX_RGBA8_UNORM, TEX_RGBA8_SRGB = 0, 1, 2
TEX_REPEAT, TEX_CLAMP = 0, 1
TEX_NEAREST, TEX_BILINEAR = 0, 1
TEX_FORMATS = dict(rgba32f=TEX_RGBA32F, rgba8_unorm=TEX_RGBA8_UNORM, rgba8_srgb=TEX_RGBA8_SRGB)
TEX_WRAPS = dict(repeat=TEX_REPEAT, clamp=TEX_CLAMP)
TEX_FILTERS = dict(nearest=TEX_NEAREST, bilinear=TEX_BILINEAR)
TEXTURE_DTYPE = np.dtype([("offset", "<u8"), ("width", "<i4"), ("height", "<i4"), ("format", "<i4"), ("wrap_s", "<i4"), ("wrap_t", "<i4"), ("filter", "<i4")])  # glrtx_texture


def pack_textures(textures):
    """A texture set as the C calls take it.  textures: a list of (array, format, wrap, filter) -- array (height, width, 3 or 4), row 0 at t = 0, float32 for
    rgba32f and uint8 for the 8-bit formats (three channels get an alpha of 1 / 255, which only a cutout on channel 3 reads); format, wrap and filter are TEX_* numbers or their
    names, wrap may be a pair (wrap_s, wrap_t).  A pair (descriptors, blob) already packed passes through.  Returns (descriptors (n,) TEXTURE_DTYPE, blob uint8)."""
    if isinstance(textures, tuple) and len(textures) == 2 and getattr(textures[0], "dtype", None) == TEXTURE_DTYPE:
        return np.ascontiguousarray(textures[0]), np.ascontiguousarray(textures[1], dtype=np.uint8).reshape(-1)
    code = lambda v, names: names[v] if isinstance(v, str) else int(v)
    desc = np.zeros(len(textures), TEXTURE_DTYPE)
    parts, at = [], 0
    for k, (arr, fmt, wrap, filt) in enumerate(textures):
        fmt = code(fmt, TEX_FORMATS)
        ws, wt = wrap if isinstance(wrap, (tuple, list)) else (wrap, wrap)
        a = np.asarray(arr)
        if a.ndim != 3 or a.shape[2] not in (3, 4):
            raise ValueError(f"pack_textures: texture {k} must be (height, width, 3 or 4), got {a.shape}")
        a = np.ascontiguousarray(a, dtype=np.float32 if fmt == TEX_RGBA32F else np.uint8)
        if a.shape[2] == 3:
            a = np.concatenate([a, np.full(a.shape[:2] + (1,), 1.0 if fmt == TEX_RGBA32F else 255, a.dtype)], axis=2)
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        desc[k] = (at, a.shape[1], a.shape[0], fmt, code(ws, TEX_WRAPS), code(wt, TEX_WRAPS), code(filt, TEX_FILTERS))
        pad = (-raw.size) % 16
        parts += [raw, np.zeros(pad, np.uint8)]
        at += raw.size + pad
    return desc, (np.concatenate(parts) if parts else np.zeros(0, np.uint8))


def srgb_table():
    """glrt_srgb_table: the 256 floats TEX_RGBA8_SRGB decodes a byte with."""
    return np.ctypeslib.as_array(lib().glrt_srgb_table(), shape=(256,)).copy()


def texture_lookup(textures, which, st):
    """glrt_texture_lookup: the CPU statement of the device's texture lookup (include/glrtx.h "Textures").  textures as pack_textures takes them; which (n,) texture
    indices; st (n, 2).  Returns rgb (n, 3) float32."""
    desc, blob = pack_textures(textures)
    w = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
    c = _f32(st).reshape(-1, 2)
    if c.shape[0] != w.size:
        raise ValueError(f"texture_lookup: {w.size} texture indices, {c.shape[0]} coordinates")
    out = np.zeros((w.size, 3), np.float32)
    rc = lib().glrt_texture_lookup(desc.ctypes.data, desc.size, blob.ctypes.data, blob.size, _ptr(w, C.c_int32), _ptr(c, C.c_float), w.size, _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_texture_lookup failed: {rc}")
    return out


def texture_albedo(scene, textures, material_texture, hits):
    """glrt_texture_albedo: what plane A of the feature pass holds for hit records as plane G stores them (hits (..., 4): wire triangle as int32 bits, u, v, 0) on
    `scene` (vert / tri / mat) with material m bound to texture material_texture[m] (-1: none).  Returns rgb (..., 3) float32."""
    desc, blob = pack_textures(textures)
    v, t, m = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["tri"]).reshape(-1, 4), _f32(scene["mat"]).reshape(-1, 18)
    b = np.ascontiguousarray(material_texture, dtype=np.int32).reshape(-1)
    if b.size != m.shape[0]:
        raise ValueError(f"texture_albedo: {m.shape[0]} materials, {b.size} bindings")
    h = _f32(hits)
    flat = h.reshape(-1, 4)
    out = np.zeros((flat.shape[0], 3), np.float32)
    rc = lib().glrt_texture_albedo(_ptr(v, C.c_float), v.shape[0], _ptr(t, C.c_float), t.shape[0], _ptr(m, C.c_float), m.shape[0], desc.ctypes.data, desc.size,
                                   blob.ctypes.data, blob.size, _ptr(b, C.c_int32), _ptr(flat, C.c_float), flat.shape[0], _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_texture_albedo failed: {rc}")
    return out.reshape(h.shape[:-1] + (3,))


# --------------------------------------------------------------------------- cutouts (include/glrtx.h "Cutouts")
CUTOUT_DTYPE = np.dtype([("texture", "<i4"), ("channel", "<i4"), ("cutoff", "<f4"), ("reserved", "<i4")])  # glrtx_cutout


def cutouts(n_mat, texture=None, channel=None, cutoff=None):
    """(n_mat,) CUTOUT_DTYPE records from per-material arrays (or scalars): texture indices of the bound set (-1 or None: not cut), channels 0 .. 3 (default 3,
    alpha) and cutoffs (default 0.5)."""
    r = np.zeros(int(n_mat), CUTOUT_DTYPE)
    r["texture"] = -1 if texture is None else np.asarray(texture, np.int32)
    r["channel"] = 3 if channel is None else np.asarray(channel, np.int32)
    r["cutoff"] = 0.5 if cutoff is None else np.asarray(cutoff, np.float32)
    return r


def texture_channel(textures, which, channel, st):
    """glrt_texture_channel: the CPU statement of the device's one-channel lookup (include/glrtx.h "Cutouts").  textures as pack_textures takes them; which (n,)
    texture indices; channel (n,) or one number, 0 .. 3; st (n, 2).  Returns (n,) float32."""
    desc, blob = pack_textures(textures)
    w = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
    ch = np.ascontiguousarray(np.broadcast_to(np.asarray(channel, np.int32), w.shape))
    c = _f32(st).reshape(-1, 2)
    if c.shape[0] != w.size:
        raise ValueError(f"texture_channel: {w.size} texture indices, {c.shape[0]} coordinates")
    out = np.zeros(w.size, np.float32)
    rc = lib().glrt_texture_channel(desc.ctypes.data, desc.size, blob.ctypes.data, blob.size, _ptr(w, C.c_int32), _ptr(ch, C.c_int32), _ptr(c, C.c_float), w.size,
                                    _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_texture_channel failed: {rc}")
    return out


# --------------------------------------------------------------------------- emission maps (include/glrtx.h "Emission maps")
def light_st(scene):
    """glrt_light_st: the device's per-light coordinate table -- (n_light, 3, 2) float32, the uv words of every light's three vertices in wire order."""
    v, l = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["light"]).reshape(-1, 4)
    out = np.zeros((l.shape[0], 3, 2), np.float32)
    rc = lib().glrt_light_st(_ptr(v, C.c_float), v.shape[0], _ptr(l, C.c_float), l.shape[0], _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_light_st failed: {rc}")
    return out


def light_emission(scene, textures, material_emission, lid, u):
    """glrt_light_emission: the CPU statement of next-event estimation's side of an emission map.  scene (vert / light / mat), textures as pack_textures takes
    them, material_emission one texture index a material (-1: none), lid (n,) light indices, u (n, 2) the RAW uniforms (the flip is taken inside).  Returns
    (n, 5) float32 {s, t, Le.rgb}."""
    desc, blob = pack_textures(textures)
    v, l, m = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["light"]).reshape(-1, 4), _f32(scene["mat"]).reshape(-1, 18)
    b = np.ascontiguousarray(material_emission, dtype=np.int32).reshape(-1)
    if b.size != m.shape[0]:
        raise ValueError(f"light_emission: {m.shape[0]} materials, {b.size} bindings")
    k = np.ascontiguousarray(lid, dtype=np.int32).reshape(-1)
    uu = _f32(u).reshape(-1, 2)
    if uu.shape[0] != k.size:
        raise ValueError(f"light_emission: {k.size} lights, {uu.shape[0]} uniform pairs")
    out = np.zeros((k.size, 5), np.float32)
    rc = lib().glrt_light_emission(_ptr(v, C.c_float), v.shape[0], _ptr(l, C.c_float), l.shape[0], _ptr(m, C.c_float), m.shape[0], desc.ctypes.data, desc.size,
                                   blob.ctypes.data, blob.size, _ptr(b, C.c_int32), _ptr(k, C.c_int32), _ptr(uu, C.c_float), k.size, _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_light_emission failed: {rc}")
    return out


def emission_albedo(scene, textures, material_texture, material_emission, hits):
    """glrt_emission_albedo: what plane A of the feature pass holds while emission maps are bound, for hit records as plane G stores them: texture_albedo, and
    the looked-up texel (without the emission) at a hit on a bound material that is not diffuse.  Returns rgb (..., 3) float32."""
    desc, blob = pack_textures(textures)
    v, t, m = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["tri"]).reshape(-1, 4), _f32(scene["mat"]).reshape(-1, 18)
    b = np.ascontiguousarray(material_texture, dtype=np.int32).reshape(-1)
    e = np.ascontiguousarray(material_emission, dtype=np.int32).reshape(-1)
    if b.size != m.shape[0] or e.size != m.shape[0]:
        raise ValueError(f"emission_albedo: {m.shape[0]} materials, {b.size} and {e.size} bindings")
    h = _f32(hits)
    flat = h.reshape(-1, 4)
    out = np.zeros((flat.shape[0], 3), np.float32)
    rc = lib().glrt_emission_albedo(_ptr(v, C.c_float), v.shape[0], _ptr(t, C.c_float), t.shape[0], _ptr(m, C.c_float), m.shape[0], desc.ctypes.data, desc.size,
                                    blob.ctypes.data, blob.size, _ptr(b, C.c_int32), _ptr(e, C.c_int32), _ptr(flat, C.c_float), flat.shape[0], _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_emission_albedo failed: {rc}")
    return out.reshape(h.shape[:-1] + (3,))


def emission_bind_check(scene, n_tex, material_emission, cutouts_bound=False):
    """glrt_emission_bind_check: what glrtx_bind_emission_maps would refuse of these bindings on `scene` with a set of n_tex textures bound -- the device's
    message behind its "glrtx_bind_emission_maps: ", or "" when the bindings may be bound."""
    m = _f32(scene["mat"]).reshape(-1, 18)
    b = np.ascontiguousarray(material_emission, dtype=np.int32).reshape(-1)
    msg = C.create_string_buffer(256)
    rc = lib().glrt_emission_bind_check(_ptr(m, C.c_float), m.shape[0], int(n_tex), int(bool(cutouts_bound)), _ptr(b, C.c_int32), b.size, msg, 256)
    text = msg.value.decode()
    if (rc == 0) != (text == ""):
        raise RuntimeError(f"glrt_emission_bind_check: {rc} with the message {text!r}")
    return text


ROUTE_KINDS = ("ordinary", "adaptive", "moments", "calibration", "adaptive_moments", "cascades")  # GLRT_ROUTE_*: the device's render calls


class RouteState(C.Structure):
    """glrt_route_state: the context fields and parameters that decide a launch's route."""
    _fields_ = [(k, C.c_int32) for k in ("variant", "ext_flags", "n_spheres", "n_tex", "n_vine", "have_volume", "have_maps", "have_cut", "have_emit", "have_env",
                                         "vol_switch", "tex_switch", "max_depth", "n_samples")]


class Route(C.Structure):
    """glrt_route"""
    _fields_ = [(k, C.c_int32) for k in ("family", "variant_last", "fallback_last", "fallback_counts", "form")] + [("kernel", C.c_char * 96)]


def launch_route(state, kind="ordinary"):
    """glrt_launch_route: the route of a render call (`kind`: one of ROUTE_KINDS) on a context in `state` -- a RouteState, or a dict of its fields (variant
    defaults to 2, max_depth to 2, n_samples to 1, the rest to 0).  Returns (route, refusal): the Route and "", or None and the device's message behind its
    "<function>: " when the call refuses."""
    if not isinstance(state, RouteState):
        state = RouteState(**{"variant": 2, "max_depth": 2, "n_samples": 1, **{k: int(v) for k, v in state.items()}})
    out, msg = Route(), C.create_string_buffer(320)
    rc = lib().glrt_launch_route(C.byref(state), ROUTE_KINDS.index(kind) if isinstance(kind, str) else int(kind), C.byref(out), msg, 320)
    text = msg.value.decode()
    if rc not in (0, -1) or (rc == 0) != (text == ""):
        raise RuntimeError(f"glrt_launch_route: {rc} with the message {text!r}")
    return (out, "") if rc == 0 else (None, text)


def render_features_geom_cutout(scene, params, textures, material_texture, cut, width=None, height=None, rank=0, world=1, stripe=16):
    """glrt_render_features_geom_cutout: render_features_geom with the cutout rule inside its closest-hit search -- the CPU statement of the feature pass under
    Device.track_motion with a set (textures, material_texture: per-material texture indices, -1 none) and cutouts (cut: (n_mat,) CUTOUT_DTYPE) bound.  Returns
    (normal_depth, albedo_id, geom) as render_features_geom does."""
    w, h = int(width or params["width"]), int(height or params["height"])
    vert, tri = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["tri"]).reshape(-1, 4)
    nodes, mat = _f32(scene["bvh"]).reshape(-1, 9), _f32(scene["mat"]).reshape(-1, 18)
    c2w, s2c = _f32(params["c2w"]).reshape(16), _f32(params["s2c"]).reshape(16)
    desc, blob = pack_textures(textures)
    b = np.ascontiguousarray(material_texture, dtype=np.int32).reshape(-1)
    rec = np.ascontiguousarray(cut, dtype=CUTOUT_DTYPE).reshape(-1)
    if b.size != mat.shape[0] or rec.size != mat.shape[0]:
        raise ValueError(f"render_features_geom_cutout: {mat.shape[0]} materials, {b.size} bindings, {rec.size} cutout records")
    rows = sum(1 for y in range(h) if (y // stripe) % world == rank)
    n, a, g = (np.zeros((rows, w, 4), np.float32) for _ in range(3))
    rc = lib().glrt_render_features_geom_cutout(_fp(vert), vert.shape[0], _fp(tri), tri.shape[0], _fp(nodes), nodes.shape[0], _fp(mat), mat.shape[0], _fp(c2w),
                                                _fp(s2c), w, h, rank, world, stripe, desc.ctypes.data, desc.size, blob.ctypes.data, blob.size, _ptr(b, C.c_int32),
                                                rec.ctypes.data, _fp(n), _fp(a), _fp(g))
    if rc != 0:
        raise RuntimeError(f"glrt_render_features_geom_cutout failed: {rc}")
    return n, a, g


# --------------------------------------------------------------------------- surface context (include/glrt_host.h "Surface context")
class Surface:
    """glrt_surface_create: the albedo, cutout and emission-map lookups of `scene` (vert / tri / light / mat, as uploaded) as per-hit C calls.  textures as
    pack_textures takes them; material_texture / material_emission one texture index a material (-1 none), cut (n_mat,) CUTOUT_DTYPE records; each may be
    None.  hooks() is what oracle.pt_oracle.render(..., surface=...) takes: the addresses of the C calls, no Python runs per hit.  albedo / accept /
    emission call them once from Python, for tests of the statements.  Use as a context manager, or close()."""

    def __init__(self, scene, textures, material_texture=None, cut=None, material_emission=None):
        desc, blob = pack_textures(textures)
        v, t, m = _f32(scene["vert"]).reshape(-1, 15), _f32(scene["tri"]).reshape(-1, 4), _f32(scene["mat"]).reshape(-1, 18)
        l = _f32(scene["light"]).reshape(-1, 4)

        def per_material(a, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            if a.size != m.shape[0]:
                raise ValueError(f"Surface: {m.shape[0]} materials, {a.size} {what}")
            return a

        b = per_material(material_texture, np.int32, "texture bindings")
        e = per_material(material_emission, np.int32, "emission bindings")
        rec = per_material(cut, CUTOUT_DTYPE, "cutout records")
        self._ctx = C.c_void_p()
        rc = lib().glrt_surface_create(_fp(v), v.shape[0], _fp(t), t.shape[0], _fp(l), l.shape[0], _fp(m), m.shape[0], desc.ctypes.data, desc.size, blob.ctypes.data,
                                       blob.size, None if b is None else _ptr(b, C.c_int32), None if rec is None else rec.ctypes.data,
                                       None if e is None else _ptr(e, C.c_int32), C.byref(self._ctx))
        if rc != 0:
            self._ctx = C.c_void_p()
            raise RuntimeError(f"glrt_surface_create failed: {rc}")

    def hooks(self, albedo=True, accept=True, emission=True):
        """(user, albedo, accept, emission): the context and the addresses of glrt_surface_albedo / _accept / _emission (None for one switched off)"""
        if not self._ctx:
            raise RuntimeError("Surface: closed")
        L = lib()
        addr = lambda f, on: C.cast(f, C.c_void_p).value if on else None
        return self._ctx.value, addr(L.glrt_surface_albedo, albedo), addr(L.glrt_surface_accept, accept), addr(L.glrt_surface_emission, emission)

    def albedo(self, tri, u, v):
        """(bound, rgb (3,) float32) of glrt_surface_albedo"""
        out = np.zeros(3, np.float32)
        return bool(lib().glrt_surface_albedo(self._ctx, int(tri), float(u), float(v), _fp(out))), out

    def accept(self, tri, u, v):
        return bool(lib().glrt_surface_accept(self._ctx, int(tri), float(u), float(v)))

    def emission(self, index, light, u, v):
        """(bound, texel (3,) float32) of glrt_surface_emission"""
        out = np.zeros(3, np.float32)
        return bool(lib().glrt_surface_emission(self._ctx, int(index), int(bool(light)), float(u), float(v), _fp(out))), out

    def close(self):
        if self._ctx:
            lib().glrt_surface_free(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------- material maps (include/glrtx.h "Material maps")
MAP_ALPHA_MIN = np.float32(1e-3)  # GLRT_MAP_ALPHA_MIN
MAP_RECORD_FLOATS = 18  # GLRT_MAP_RECORD_FLOATS: {n, e1, e2, (s0, t0), (s1, t1), (s2, t2), m}
MATERIAL_MAP_DTYPE = np.dtype([("normal", "<i4"), ("roughness", "<i4"), ("normal_scale", "<f4"), ("reserved", "<i4")])  # glrtx_material_map


def material_maps(n_mat, normal=None, roughness=None, normal_scale=1.0):
    """(n_mat,) MATERIAL_MAP_DTYPE records from per-material arrays (or scalars): texture indices of the bound set, -1 or None for no map."""
    r = np.zeros(int(n_mat), MATERIAL_MAP_DTYPE)
    r["normal"] = -1 if normal is None else np.asarray(normal, np.int32)
    r["roughness"] = -1 if roughness is None else np.asarray(roughness, np.int32)
    r["normal_scale"] = np.asarray(normal_scale, np.float32)
    return r


def map_records(n, e1, e2, st0, st1, st2, m):
    """(k, MAP_RECORD_FLOATS) float32 records of glrt_map_normal / glrtx_debug_map_normal from arrays of shape (k, 3) and (k, 2), words moved as they are."""
    parts = [np.ascontiguousarray(a, np.float32).reshape(-1, w) for a, w in ((n, 3), (e1, 3), (e2, 3), (st0, 2), (st1, 2), (st2, 2), (m, 3))]
    return np.ascontiguousarray(np.concatenate([p.view(np.uint32) for p in parts], 1)).view(np.float32)


def _map_call(name, src, width_in, width_out, *extra):
    a = np.ascontiguousarray(src, np.float32).reshape(-1, width_in)
    out = np.zeros((a.shape[0], width_out), np.float32)
    rc = getattr(lib(), name)(_ptr(a, C.c_float), a.shape[0], *extra, _ptr(out, C.c_float))
    if rc:
        raise RuntimeError(f"{name} failed: {rc}")
    return out


def map_decode(rgb):
    """glrt_map_decode: looked-up texels (k, 3) as tangent-space vectors, m = c * 2 + -1."""
    return _map_call("glrt_map_decode", rgb, 3, 3)


def map_normal(records, scale=1.0):
    """glrt_map_normal: the CPU statement of the device's tangent-space normal rule; records as map_records makes them, returns n' (k, 3) float32."""
    return _map_call("glrt_map_normal", records, MAP_RECORD_FLOATS, 3, C.c_float(scale))


def map_alpha(rgb):
    """glrt_map_alpha: (alpha.x, alpha.y) (k, 2) of roughness texels (k, 3): channels r and g, floored at MAP_ALPHA_MIN."""
    return _map_call("glrt_map_alpha", rgb, 3, 2)


REPROJECT_DEFAULTS = dict(max_history=32, depth_tolerance=0.02, normal_tolerance=0.9)


def reproject(accum, n0, a0, n1, a1, prev, cur, max_history=REPROJECT_DEFAULTS["max_history"], depth_tolerance=REPROJECT_DEFAULTS["depth_tolerance"],
              normal_tolerance=REPROJECT_DEFAULTS["normal_tolerance"]):
    """glrt_reproject: the CPU statement of Device.reproject on (rows, width, 4) float32 arrays.  accum, n0, a0: the old view's accumulator and feature planes;
    n1, a1: the new view's planes; prev / cur: the two cameras (dicts with c2w and s2c).  Returns (out, carried, hit_pixels)."""
    arr = [_f32(v) for v in (accum, n0, a0, n1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"reproject: five (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    mats = [_f32(m).reshape(16) for m in (prev["c2w"], prev["s2c"], cur["c2w"], cur["s2c"])]
    out = np.zeros_like(a)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = lib().glrt_reproject(*[_fp(v) for v in arr], *[_fp(m) for m in mats], a.shape[1], a.shape[0], int(max_history), float(depth_tolerance),
                              float(normal_tolerance), _fp(out), C.byref(carried), C.byref(hits))
    if rc != 0:
        raise RuntimeError(f"glrt_reproject failed: {rc}")
    return out, int(carried.value), int(hits.value)


def reproject_motion(accum, n0, a0, g1, a1, vert_prev, tri, prev, max_history=REPROJECT_DEFAULTS["max_history"],
                     depth_tolerance=REPROJECT_DEFAULTS["depth_tolerance"], normal_tolerance=REPROJECT_DEFAULTS["normal_tolerance"]):
    """glrt_reproject_motion: the CPU statement of Device.reproject_motion on (rows, width, 4) float32 arrays.  accum, n0, a0: the old view's accumulator and
    feature planes; g1, a1: the new view's geometry and albedo planes; vert_prev: the vertices as they stood at the old view; tri: the scene's triangles;
    prev: the old view's camera (a dict with c2w and s2c).  Returns (out, carried, hit_pixels)."""
    arr = [_f32(v) for v in (accum, n0, a0, g1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"reproject_motion: five (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    vert, tr = _f32(vert_prev).reshape(-1, 15), _f32(tri).reshape(-1, 4)
    mats = [_f32(m).reshape(16) for m in (prev["c2w"], prev["s2c"])]
    out = np.zeros_like(a)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = lib().glrt_reproject_motion(*[_fp(v) for v in arr], _fp(vert), vert.shape[0], _fp(tr), tr.shape[0], *[_fp(m) for m in mats], a.shape[1], a.shape[0],
                                     int(max_history), float(depth_tolerance), float(normal_tolerance), _fp(out), C.byref(carried), C.byref(hits))
    if rc != 0:
        raise RuntimeError(f"glrt_reproject_motion failed: {rc}")
    return out, int(carried.value), int(hits.value)


def reproject_moments(accum, moments, n0, a0, n1, a1, prev, cur, max_history=REPROJECT_DEFAULTS["max_history"],
                      depth_tolerance=REPROJECT_DEFAULTS["depth_tolerance"], normal_tolerance=REPROJECT_DEFAULTS["normal_tolerance"]):
    """glrt_reproject_moments: reproject with the old view's moments plane M carried through the same taps (the CPU statement of Device.reproject while
    Device.track_moments is on).  Returns (out, moments_out, carried, hit_pixels)."""
    arr = [_f32(v) for v in (accum, moments, n0, a0, n1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"reproject_moments: six (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    mats = [_f32(m).reshape(16) for m in (prev["c2w"], prev["s2c"], cur["c2w"], cur["s2c"])]
    out, mo = np.zeros_like(a), np.zeros_like(a)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = lib().glrt_reproject_moments(*[_fp(v) for v in arr], *[_fp(m) for m in mats], a.shape[1], a.shape[0], int(max_history), float(depth_tolerance),
                                      float(normal_tolerance), _fp(out), _fp(mo), C.byref(carried), C.byref(hits))
    if rc != 0:
        raise RuntimeError(f"glrt_reproject_moments failed: {rc}")
    return out, mo, int(carried.value), int(hits.value)


def reproject_motion_moments(accum, moments, n0, a0, g1, a1, vert_prev, tri, prev, max_history=REPROJECT_DEFAULTS["max_history"],
                             depth_tolerance=REPROJECT_DEFAULTS["depth_tolerance"], normal_tolerance=REPROJECT_DEFAULTS["normal_tolerance"]):
    """glrt_reproject_motion_moments: reproject_motion with the old view's moments plane M carried.  Returns (out, moments_out, carried, hit_pixels)."""
    arr = [_f32(v) for v in (accum, moments, n0, a0, g1, a1)]
    a = arr[0]
    if a.ndim != 3 or a.shape[2] != 4 or any(v.shape != a.shape for v in arr):
        raise ValueError(f"reproject_motion_moments: six (rows, width, 4) arrays of one shape expected, got {[v.shape for v in arr]}")
    vert, tr = _f32(vert_prev).reshape(-1, 15), _f32(tri).reshape(-1, 4)
    mats = [_f32(m).reshape(16) for m in (prev["c2w"], prev["s2c"])]
    out, mo = np.zeros_like(a), np.zeros_like(a)
    carried, hits = C.c_int(0), C.c_int(0)
    rc = lib().glrt_reproject_motion_moments(*[_fp(v) for v in arr], _fp(vert), vert.shape[0], _fp(tr), tr.shape[0], *[_fp(m) for m in mats], a.shape[1],
                                             a.shape[0], int(max_history), float(depth_tolerance), float(normal_tolerance), _fp(out), _fp(mo), C.byref(carried),
                                             C.byref(hits))
    if rc != 0:
        raise RuntimeError(f"glrt_reproject_motion_moments failed: {rc}")
    return out, mo, int(carried.value), int(hits.value)


def look_at(eye, center, up) -> np.ndarray:
    out = np.zeros(16, np.float32)
    lib().glrt_look_at(_fp(_f32(eye)), _fp(_f32(center)), _fp(_f32(up)), _fp(out))
    return out


def perspective(fovy_deg, aspect, z_near, z_far) -> np.ndarray:
    out = np.zeros(16, np.float32)
    lib().glrt_perspective(fovy_deg, aspect, z_near, z_far, _fp(out))
    return out


# Environment (include/glrtx.h "Environment"): GLRTX_ENV_*
ENV_ESCAPE, ENV_SAMPLED = 0, 1
ENV_MODES = dict(escape=ENV_ESCAPE, sampled=ENV_SAMPLED)


class EnvCfg(C.Structure):  # glrtx_env_cfg == glrt_env_cfg
    _fields_ = [("mode", C.c_int32), ("grid", C.c_int32), ("light_pick", C.c_float), ("scale", C.c_float * 3), ("rotation", C.c_float * 9)]


def env_cfg(mode=ENV_ESCAPE, grid=0, light_pick=0.5, scale=1.0, rotation=None, rotate_y=None) -> EnvCfg:
    """A glrtx_env_cfg.  mode: ENV_* or its name; scale: a number or an RGB triple; rotation: a row-major 3 x 3 (map space = rotation * world), default the
    identity; rotate_y (degrees) instead: the map turned about +y, so that what lay along +z lies along +x after a quarter turn."""
    c = EnvCfg()
    c.mode = ENV_MODES[mode] if isinstance(mode, str) else int(mode)
    c.grid = int(grid)
    c.light_pick = float(light_pick)
    c.scale[:] = [float(v) for v in np.broadcast_to(np.asarray(scale, np.float32), (3,))]
    if rotation is None:
        a = np.deg2rad(0.0 if rotate_y is None else float(rotate_y))
        cs, sn = np.float32(np.cos(a)), np.float32(np.sin(a))
        if rotate_y is not None and float(rotate_y) % 90.0 == 0.0:  # quarter turns exactly
            cs, sn = np.float32(round(float(np.cos(a)))), np.float32(round(float(np.sin(a))))
        rotation = [cs, 0.0, 0.0 - sn, 0.0, 1.0, 0.0, sn, 0.0, cs]  # (0 - 0 = +0: no turn is the identity's words)
    c.rotation[:] = [float(v) for v in np.asarray(rotation, np.float32).reshape(9)]
    return c


def pack_environment(env_map):
    """An environment map as the C calls take it.  env_map: (array, format, filter) -- array (N, N, 3 or 4) as pack_textures takes a texture, row 0 at t = 0
    (the -z edge of the octahedral square), clamp on both axes.  A pair (descriptors, blob) already packed passes through."""
    if isinstance(env_map, tuple) and len(env_map) == 2 and getattr(env_map[0], "dtype", None) == TEXTURE_DTYPE:
        return pack_textures(env_map)
    arr, fmt, filt = env_map
    return pack_textures([(arr, fmt, TEX_CLAMP, filt)])


def _env_call(name, env_map, cfg, *rest):
    desc, blob = pack_environment(env_map)
    rc = getattr(lib(), name)(desc.ctypes.data, blob.ctypes.data, blob.size, C.addressof(cfg) if cfg is not None else None, *rest)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {rc}")


def env_weights(env_map, cfg):
    """glrt_env_weights: the importance grid's cell weights, (G, G) float32 with row j (the t axis) first, in the device's summation order."""
    desc, _ = pack_environment(env_map)
    g = int(cfg.grid) if cfg is not None and 0 < int(cfg.grid) <= 1024 else min(int(desc["width"][0]), 256)
    out, grid = np.zeros(max(g, 1) ** 2, np.float32), C.c_int32(0)
    _env_call("glrt_env_weights", env_map, cfg, _ptr(out, C.c_float), C.byref(grid))
    return out.reshape(grid.value, grid.value)


def env_alias(weights):
    """glrt_env_alias: the sampling tables of a (G, G) grid of weights.  Returns dict(row_q (G,), row_alias (G,), col_q (G, G), col_alias (G, G), cell_p (G, G))."""
    w = _f32(weights)
    if w.ndim != 2 or w.shape[0] != w.shape[1]:
        raise ValueError(f"env_alias: weights must be (G, G), got {w.shape}")
    g = w.shape[0]
    t = dict(row_q=np.zeros(g, np.float32), row_alias=np.zeros(g, np.int32), col_q=np.zeros((g, g), np.float32), col_alias=np.zeros((g, g), np.int32),
             cell_p=np.zeros((g, g), np.float32))
    rc = lib().glrt_env_alias(_ptr(w, C.c_float), g, _ptr(t["row_q"], C.c_float), _ptr(t["row_alias"], C.c_int32), _ptr(t["col_q"], C.c_float),
                              _ptr(t["col_alias"], C.c_int32), _ptr(t["cell_p"], C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_env_alias failed: {rc}")
    return t


def env_sample(env_map, cfg, u):
    """glrt_env_sample: six uniforms a row of u (n, 6) -> (n, 8) float32 rows {direction, pdf, Le.rgb, 0}; the pdf carries p_env = cfg.light_pick."""
    q = _f32(u).reshape(-1, 6)
    out = np.zeros((q.shape[0], 8), np.float32)
    _env_call("glrt_env_sample", env_map, cfg, _ptr(q, C.c_float), q.shape[0], _ptr(out, C.c_float))
    return out


def env_eval(env_map, cfg, dirs):
    """glrt_env_eval: directions (n, 3), not normalised -> (n, 4) float32 rows {Le.rgb, pdf}."""
    d = _f32(dirs).reshape(-1, 3)
    out = np.zeros((d.shape[0], 4), np.float32)
    _env_call("glrt_env_eval", env_map, cfg, _ptr(d, C.c_float), d.shape[0], _ptr(out, C.c_float))
    return out


def env_from_latlong(image, n):
    """glrt_env_from_latlong: a lat-long image (height, width, 3) -- +y up, the top row +y, the centre column -z -- resampled into an (n, n, 4) float32
    octahedral map (alpha 1)."""
    a = _f32(np.asarray(image)[..., :3])
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"env_from_latlong: image must be (height, width, 3 or 4), got {np.asarray(image).shape}")
    out = np.zeros((int(n), int(n), 4), np.float32)
    rc = lib().glrt_env_from_latlong(_ptr(a, C.c_float), a.shape[1], a.shape[0], int(n), _ptr(out, C.c_float))
    if rc != 0:
        raise RuntimeError(f"glrt_env_from_latlong failed: {rc}")
    return out


def mat4_inverse(m) -> np.ndarray:
    out = np.zeros(16, np.float32)
    if lib().glrt_mat4_inverse(_fp(_f32(m)), _fp(out)) != 0:
        raise RuntimeError("singular matrix")
    return out


def mat4_mul(a, b) -> np.ndarray:
    out = np.zeros(16, np.float32)
    lib().glrt_mat4_mul(_fp(_f32(a)), _fp(_f32(b)), _fp(out))
    return out


def frame_seed(frame: int):
    out = np.zeros(2, np.float32)
    lib().glrt_frame_seed(frame, _fp(out))
    return float(out[0]), float(out[1])
