"""numpy statement of the deform pass over a sparse morph-target set (include/glrtx.h "Deforming", SPARSE TARGETS; csrc/skin.hip.h: deform_sparse_kernel;
host/deform.cpp: glrt_deform_vertices_sparse), and the index patterns the tests turn deform_math's hostile deltas into.

The rules and the skinning stage are deform_math's, imported and unchanged.  The morph walks the targets in ascending index and adds each active one's entries to
the vertices they list: per vertex that is "the entries that list this vertex and belong to an active target, in ascending target index".  A vertex no active
target lists keeps its rest words -- nothing is added to it, not even a zero.
"""
from __future__ import annotations

import numpy as np

import deform_math as dm
import skin_math as sm
from adaptive_math import _op
from skin_math import add, mul

MAX_SPARSE_TARGETS = 1024
TARGETS = [0, 1, 3, 64, 65, 1024]
PATTERNS = ["all", "random5", "first", "last", "one_vertex", "empty_targets", "inactive_nan"]


def morph(rest, offsets, vertex, deltas, morph_weights):
    r = np.ascontiguousarray(rest, np.float32).reshape(-1, 15)
    pn = r[:, 0:6].copy()
    if morph_weights is None:
        return pn[:, 0:3], pn[:, 3:6]
    o = np.asarray(offsets, np.uint64).astype(np.int64)
    v = np.asarray(vertex, np.uint32).astype(np.int64)
    d = np.asarray(deltas, np.float32).reshape(-1, 6)
    w = np.asarray(morph_weights, np.float32).reshape(-1)
    for k in dm.active_targets(w):
        idx = v[o[k]:o[k + 1]]  # strictly ascending: no vertex twice
        if idx.size:
            pn[idx] = _op(add, pn[idx], _op(mul, w[k], d[o[k]:o[k + 1]]))
    return pn[:, 0:3], pn[:, 3:6]


def deform(rest, bones, weights, bone_data, mode=0, offsets=None, vertex=None, deltas=None, morph_weights=None):
    """The deformed vertices (n, 15) float32: the sparse morph, then deform_math's skinning stage."""
    p, n = morph(rest, offsets, vertex, deltas, morph_weights)
    B = dm.dualquat_matrix(bones, weights, bone_data) if mode else sm.blend(bones, weights, bone_data)
    return dm.transform(rest, p, n, B)


def from_mask(dense, mask):
    """(offsets, vertex, deltas) of the entries of dense (T, n, 6) that mask (T, n) keeps."""
    dense = np.asarray(dense, np.float32)
    T = dense.shape[0]
    idx = [np.flatnonzero(mask[k]).astype(np.uint32) for k in range(T)]
    offsets = np.zeros(T + 1, np.uint64)
    offsets[1:] = np.cumsum([i.size for i in idx], dtype=np.uint64)
    vertex = np.concatenate(idx) if T else np.zeros(0, np.uint32)
    deltas = np.concatenate([dense[k, idx[k]] for k in range(T)]) if T else np.zeros((0, 6), np.float32)
    return offsets, vertex.astype(np.uint32), np.ascontiguousarray(deltas, np.float32).reshape(-1, 6)


def pattern(name, dense, mw, seed):
    """(offsets, vertex, deltas, morph_weights) for one index pattern over the hostile dense deltas (T, n, 6) and their weights.
    all: every vertex in every target; random5: a random 5 %; first / last: only vertex 0 / n - 1; one_vertex: one vertex listed by all targets, every other
    row empty; empty_targets: a random third of the entries, every other target's list empty; inactive_nan: the only entries belong to inactive targets and
    hold NaN (the weights are this pattern's own: even targets 0, +-denormal, odd ones active with empty lists)."""
    dense = np.asarray(dense, np.float32)
    T, n = dense.shape[0:2]
    rng = np.random.default_rng(seed + 4242)
    mask = np.zeros((T, n), bool)
    if name == "all":
        mask[:] = True
    elif name == "random5":
        mask = rng.random((T, n)) < 0.05
    elif name == "first":
        mask[:, 0] = True
    elif name == "last":
        mask[:, n - 1] = True
    elif name == "one_vertex":
        mask[:, n // 2] = True
    elif name == "empty_targets":
        mask = rng.random((T, n)) < 0.33
        mask[0::2] = False
    elif name == "inactive_nan":
        mw = np.where(np.arange(T) % 2 == 0, np.array([0.0, 1e-40, -1e-40, -0.0], np.float32)[(np.arange(T) // 2) % 4], np.float32(0.75)).astype(np.float32)
        mask[0::2] = rng.random((T, n))[0::2] < 0.5
        mask[0::2, 0] = True
        dense = np.full_like(dense, np.nan)
    else:
        raise ValueError(name)
    return from_mask(dense, mask) + (np.asarray(mw, np.float32),)


def hostile_dense(n_vert, n_targets, seed):
    """deform_math.hostile_morph for up to 1024 targets: (dense (T, n, 6), morph_weights (T,)), both empty without targets."""
    if n_targets == 0:
        return np.zeros((0, n_vert, 6), np.float32), np.zeros(0, np.float32)
    return dm.hostile_morph(n_vert, n_targets, seed)


def hostile_rig(n_vert, n_bones, mode, seed):
    """deform_math.hostile_case's (rest, bones, weights, bone_data)."""
    return dm.hostile_case(n_vert, n_bones, mode, 0, seed)[0:4]


def hostile_sparse(n_vert, n_bones, mode, n_targets, seed):
    """deform_math.hostile_case with dense deltas for up to 1024 targets: (rest, bones, weights, bone_data, dense (T, n, 6), morph_weights (T,))."""
    return hostile_rig(n_vert, n_bones, mode, seed) + hostile_dense(n_vert, n_targets, seed)


def grid_cases(n_vert, mode, bones_list):
    """What the host test and the GPU test both walk for one (n_vert, mode): every n_targets of TARGETS x every pattern, one bone count a pattern (going round
    bones_list), plus every bone count once on the 3-target random set.  Yields (what, rest, bones, weights, bone_data, offsets, vertex, deltas, weights)."""
    for n_targets in TARGETS:
        dense, mw = hostile_dense(n_vert, n_targets, 1000 * n_vert)
        todo = [(name, bones_list[(j + n_targets) % len(bones_list)]) for j, name in enumerate(PATTERNS if n_targets else ["all"])]
        if n_targets == 3:
            todo += [("random5", nb) for nb in bones_list] + [("all", nb) for nb in bones_list]
        for name, n_bones in todo:
            rig = hostile_rig(n_vert, n_bones, mode, 1000 * n_vert + n_bones)
            yield (f"{n_targets} targets, {name}, {n_bones} bones", name) + rig + pattern(name, dense, mw, 1000 * n_vert + n_bones)
