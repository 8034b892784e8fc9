"""The batch of map_normal records the three statements of "Material maps" are compared on (tests/test_maps_host.py on the CPU, tests/test_gpu_maps.py on the
device): random frames and texels, then every case the contract names -- det zero, negative, inf and NaN; n parallel to Tr; m = (0, 0, 1) and (-0, 0, 1); m.z = 0;
m all zero; a scale of 0 (the caller's); non-finite texels; denormal words."""
from __future__ import annotations

import numpy as np

RECORD_FLOATS = 18
SCALES = (1.0, 0.0, -2.5, 0.37)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def record(n, e1, e2, st0, st1, st2, m):
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in (n, e1, e2, st0, st1, st2, m)])


def random_records(k=512, seed=7):
    """Triangles in general position with a shading normal within ~30 degrees of the face normal, arbitrary coordinates, texels in [0, 1] decoded."""
    rng = np.random.default_rng(seed)
    e1, e2 = rng.normal(size=(k, 3)), rng.normal(size=(k, 3))
    n = _unit(_unit(np.cross(e1, e2)) + 0.3 * rng.normal(size=(k, 3)))
    st = rng.uniform(-2.0, 3.0, (k, 3, 2))
    m = rng.uniform(0.0, 1.0, (k, 3)).astype(np.float32) * np.float32(2) + np.float32(-1)
    return np.concatenate([n, e1, e2, st[:, 0], st[:, 1], st[:, 2], m], 1).astype(np.float32)


def edge_records():
    inf, nan = np.inf, np.nan
    n, e1, e2 = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)  # the quad y = 0, s along +x, t along -z
    st = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
    tilt = (0.5, 0.25, 0.8)
    den = np.float32(1e-41)
    rows = [
        record(n, e1, e2, *st, tilt),                                             # the plain case
        record(n, e1, e2, (0.2, 0.2), (0.2, 0.2), (0.2, 0.2), tilt),              # det = 0: coordinates constant over the triangle
        record(n, e1, e2, (0.0, 0.0), (1.0, 1.0), (2.0, 2.0), tilt),              # det = 0: collinear coordinates
        record(n, e1, e2, (0.0, 0.0), (0.0, 1.0), (1.0, 0.0), tilt),              # det < 0: mirrored
        record(n, e1, e2, (0.0, 0.0), (-1.0, 0.0), (0.0, 1.0), tilt),             # det < 0: s mirrored
        record(n, e1, e2, (0.0, 0.0), (inf, 0.0), (0.0, 1.0), tilt),              # det = inf
        record(n, e1, e2, (0.0, 0.0), (3e38, 0.0), (0.0, 3e38), tilt),            # det overflows
        record(n, e1, e2, (0.0, 0.0), (nan, 0.0), (0.0, 1.0), tilt),              # det = NaN
        record(n, e1, e2, (inf, 0.0), (inf, 0.0), (0.0, 1.0), tilt),              # inf - inf
        record((1.0, 0.0, 0.0), e1, e2, *st, tilt),                               # n parallel to Tr: l2 = 0
        record((-1.0, 0.0, 0.0), e1, e2, *st, tilt),
        record(n, e1, e2, *st, (0.0, 0.0, 1.0)),                                  # flat
        record(n, e1, e2, *st, (-0.0, 0.0, 1.0)),
        record(n, e1, e2, *st, (-0.0, -0.0, 1.0)),
        record(n, e1, e2, *st, (0.6, -0.3, 0.0)),                                 # m.z = 0: n' in the tangent plane
        record(n, e1, e2, *st, (0.0, 0.0, 0.0)),                                  # m all zero
        record(n, e1, e2, *st, (0.0, 0.5, 0.0)),
        record(n, e1, e2, *st, (den, den, 1.0)),                                  # denormal a, b: flat
        record(n, e1, e2, *st, (nan, 0.1, 0.9)),                                  # non-finite texels
        record(n, e1, e2, *st, (0.1, inf, 0.9)),
        record(n, e1, e2, *st, (0.1, 0.2, -inf)),
        record(n, e1, e2, *st, (0.1, 0.2, nan)),
        record(n, e1, e2, *st, (3e38, 3e38, 3e38)),                               # q overflows
        record(n, e1, e2, *st, (1e-20, 1e-20, 1e-20)),                            # q underflows to zero
        record((nan, 1.0, 0.0), e1, e2, *st, tilt),                               # a NaN normal is kept as it is
        record((0.0, inf, 0.0), e1, e2, *st, tilt),
        record((0.0, 0.0, 0.0), e1, e2, *st, tilt),                               # a zero normal: T = Tr normalised, C = 0
        record(n, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), *st, tilt),                   # a degenerate triangle: Tr = 0
        record(n, (den, 0.0, 0.0), e2, *st, tilt),                                # a denormal edge
        record(n, (1e20, 0.0, 0.0), (0.0, 0.0, -1e20), *st, tilt),                # l2 overflows
        record(n, e1, e2, (0.0, 0.0), (1e-30, 0.0), (0.0, 1e-30), tilt),          # det underflows to zero
    ]
    return np.stack(rows).astype(np.float32)


def batch():
    return np.concatenate([random_records(), edge_records()], 0)
