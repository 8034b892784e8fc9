"""Rigs for Device.upload_rig / host.skin_vertices (include/glrtx.h "Posing"): four bone indices and four weights a vertex; and dual-quaternion poses for
Device.pose_dualquat / host.deform_vertices (include/glrtx.h "Deforming")."""
from __future__ import annotations

import numpy as np

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)  # one pose matrix: row-major 3x4


def rigid(object_of_vertex):
    """Rigid objects: vertex i follows bone object_of_vertex[i] alone.  Returns (bones (n, 4) int32 {obj, 0, 0, 0}, weights (n, 4) float32 {1, 0, 0, 0})."""
    obj = np.asarray(object_of_vertex)
    if obj.ndim != 1 or not np.issubdtype(obj.dtype, np.integer):
        raise ValueError(f"rigid: one integer object index a vertex expected, got {obj.dtype} {obj.shape}")
    bones = np.zeros((obj.size, 4), np.int32)
    bones[:, 0] = obj
    weights = np.zeros((obj.size, 4), np.float32)
    weights[:, 0] = 1.0
    return bones, weights


def identity_pose(n_bones):
    """n_bones identity matrices (n_bones, 12) float32."""
    return np.tile(IDENTITY, (int(n_bones), 1))


IDENTITY_DUALQUAT = np.array([0, 0, 0, 1, 0, 0, 0, 0], np.float32)  # {r.x, r.y, r.z, r.w, d.x, d.y, d.z, d.w}


def dualquat(matrices):
    """The dual-quaternion pose (n_bones, 8) float32 of rigid 3x4 matrices (n_bones, 12) or (n_bones, 3, 4): glrt_dualquat_from_matrix a bone (the rotation is
    taken as orthonormal, r.w >= 0)."""
    from .host import dualquat_from_matrix
    m = np.ascontiguousarray(matrices, np.float32)
    if m.size % 12 or m.size == 0:
        raise ValueError(f"dualquat: matrices must be (n_bones, 12) or (n_bones, 3, 4), got {m.shape}")
    return np.stack([dualquat_from_matrix(row) for row in m.reshape(-1, 12)])


def identity_dualquats(n_bones):
    """n_bones identity dual quaternions (n_bones, 8) float32."""
    return np.tile(IDENTITY_DUALQUAT, (int(n_bones), 1))
