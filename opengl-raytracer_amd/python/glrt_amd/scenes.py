"""Synthetic scenes in the reference's flat buffer wire format.

The reference ships no scenes (its .gitignore excludes scenes/*), so the
BASELINE.json configurations are generated here, deterministically, as the five
buffers Scene::parse uploads (scene.cpp:254-269):

  vert  (nV*5, 3)  pos, normal, uv, tangent, binormal     trimesh.h:15-25
  tri   (nT, 4)    i, j, k, materialId  (as floats)        scene.h:16-18
  mat   (nM*6, 3)  type, emission, param0, param1, param2, texIds   scene.h:28-35
  light (nL, 4)    copy of every emissive triangle         scene.cpp:246-248
  bvh   (nN*3, 3)  bboxMin, bboxMax, children              bvh.h:84-100

Like the reference's OBJ path, meshes carry three fresh vertices per triangle
(trimesh.cpp:186-187).  "Spheres" are icospheres: the reference has no analytic
sphere primitive.
"""
from __future__ import annotations

import numpy as np

from . import host

MTRL_EMITTER, MTRL_DIFFUSE, MTRL_CONDUCTOR, MTRL_DIELECTRIC, MTRL_MEDIA = 1, 2, 3, 4, 5


# --------------------------------------------------------------------------- materials
def emitter(emission):
    return dict(type=MTRL_EMITTER, emission=emission)


def diffuse(reflectance, texture=None):
    """texture (optional, for export_json_obj): the shape's "texture" block {"file": name, "filter": .., "wrap": .., "srgb": ..} (host/scene.h; read only with
    extensions on).  The buffers SceneBuilder makes do not change with it: a texture set is bound with Device.upload_textures."""
    return dict(type=MTRL_DIFFUSE, param0=reflectance, texture=texture) if texture is not None else dict(type=MTRL_DIFFUSE, param0=reflectance)


def conductor(eta, kappa, alpha):
    # scene.cpp:152-162: param0 = kappa, param1 = eta, param2 = (alpha, alpha, alpha)
    return dict(type=MTRL_CONDUCTOR, param0=kappa, param1=eta, param2=(alpha, alpha, alpha))


def media(volume=None):
    """volume (optional, for export_json_obj): the shape's "volume" block {"density": file, "temperature": file, "bboxMin": [..], "bboxMax": [..]}
    (the reference's scene.cpp:174-214; rendered only with the volume switch, include/glrtx.h GLRTX_EXT_VOLUME)."""
    return dict(type=MTRL_MEDIA, volume=volume) if volume is not None else dict(type=MTRL_MEDIA)


def _mat_rows(m):
    z = (0.0, 0.0, 0.0)
    t = float(m["type"])
    return [(t, t, t), m.get("emission", z), m.get("param0", z), m.get("param1", z), m.get("param2", z), z]


# --------------------------------------------------------------------------- meshes
def _icosahedron():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5],
                  [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    return v, f


def icosphere(subdiv: int, radius: float, center):
    """Returns (pos (nT,3,3), nrm (nT,3,3)) float32; 20*4**subdiv triangles, smooth unit normals."""
    v, f = _icosahedron()
    tris = v[f]  # (20,3,3)
    for _ in range(subdiv):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        ab /= np.linalg.norm(ab, axis=1, keepdims=True)
        bc /= np.linalg.norm(bc, axis=1, keepdims=True)
        ca /= np.linalg.norm(ca, axis=1, keepdims=True)
        tris = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1),
                               np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)], 0)
    nrm = tris.astype(np.float32)
    pos = (tris * radius + np.asarray(center, np.float64)).astype(np.float32)
    return pos, nrm


def quad(p0, e1, e2):
    """Two triangles p0, p0+e1, p0+e1+e2, p0+e2 with flat normal normalize(cross(e1, e2))."""
    p0, e1, e2 = (np.asarray(x, np.float64) for x in (p0, e1, e2))
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n)
    a, b, c, d = p0, p0 + e1, p0 + e1 + e2, p0 + e2
    pos = np.array([[a, b, c], [a, c, d]], np.float32)
    nrm = np.broadcast_to(n.astype(np.float32), pos.shape).copy()
    return pos, nrm


def random_triangles(n: int, seed: int, extent: float, size: float = 0.15):
    """centres U(-extent, extent)^3, vertices centre + size*U(-1,1)^3; flat normals."""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(-extent, extent, (n, 1, 3))
    pos = (ctr + size * rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(np.float32)
    e1 = pos[:, 1].astype(np.float64) - pos[:, 0]
    e2 = pos[:, 2].astype(np.float64) - pos[:, 0]
    nn = np.cross(e1, e2)
    ln = np.linalg.norm(nn, axis=1, keepdims=True)
    nn = np.where(ln > 0, nn / np.maximum(ln, 1e-30), np.array([0.0, 0.0, 1.0]))
    nrm = np.repeat(nn[:, None, :], 3, 1).astype(np.float32)
    return pos, nrm, rng


# --------------------------------------------------------------------------- assembly
class SceneBuilder:
    def __init__(self):
        self.materials = []
        self._pos, self._nrm, self._mid = [], [], []
        self._uv = []  # per add_mesh: None, or (nT, 3, 2) texture coordinates

    def add_material(self, m) -> int:
        self.materials.append(m)
        return len(self.materials) - 1

    def add_mesh(self, pos, nrm, material_id, uv=None):
        """uv (optional): (nT, 3, 2) texture coordinates (s, t), written into the vertices' uv row (uv.z stays 0); without it the row is zeros, as before."""
        pos = np.asarray(pos, np.float32).reshape(-1, 3, 3)
        nrm = np.asarray(nrm, np.float32).reshape(-1, 3, 3)
        self._uv.append(None if uv is None else np.asarray(uv, np.float32).reshape(pos.shape[0], 3, 2))
        mid = np.broadcast_to(np.asarray(material_id, np.float32), (pos.shape[0],))
        self._pos.append(pos)
        self._nrm.append(nrm)
        self._mid.append(mid.copy())

    def build(self, bvh: str = "sah"):
        pos = np.concatenate(self._pos, 0)
        nrm = np.concatenate(self._nrm, 0)
        mid = np.concatenate(self._mid, 0)
        n_tri = pos.shape[0]
        vert = np.zeros((n_tri * 3, 5, 3), np.float32)
        vert[:, 0] = pos.reshape(-1, 3)
        vert[:, 1] = nrm.reshape(-1, 3)
        if any(u is not None for u in self._uv):
            uv = np.concatenate([np.zeros((p.shape[0], 3, 2), np.float32) if u is None else u for p, u in zip(self._pos, self._uv)], 0)
            vert[:, 2, :2] = uv.reshape(-1, 2)
        vert = vert.reshape(-1, 3)
        idx = np.arange(n_tri * 3, dtype=np.float32).reshape(n_tri, 3)
        tri = np.concatenate([idx, mid[:, None]], 1).astype(np.float32)
        mat = np.array([r for m in self.materials for r in _mat_rows(m)], np.float32)
        emissive = np.array([float(np.linalg.norm(np.asarray(m.get("emission", (0, 0, 0)), np.float64))) != 0.0
                             for m in self.materials])
        light = tri[emissive[mid.astype(np.int64)]]
        built, depth = host.build_bvh(vert, tri, bvh)
        # the light side first (host.lights_first: glrt_bvh_lights_first, as glrt::Scene::parse applies it); `bvh_builder` keeps the builder's own output
        # (the reference host's own tree -- "reference" -- is never re-ordered: its point is the reference's own visiting order)
        nodes, swapped = host.lights_first(built, tri, mat) if bvh not in ("chain", "reference") else (built, 0)
        return dict(vert=vert, tri=tri, mat=mat, light=np.ascontiguousarray(light.reshape(-1, 4)), bvh=nodes,
                    bvh_depth=depth, bvh_kind=bvh, bvh_builder=built, bvh_lights_first=swapped)


def rebuild_bvh(scene, kind: str):
    s = dict(scene)
    s["bvh_builder"], s["bvh_depth"] = host.build_bvh(scene["vert"], scene["tri"], kind)
    s["bvh"], s["bvh_lights_first"] = host.lights_first(s["bvh_builder"], scene["tri"], scene["mat"]) if kind not in ("chain", "reference") else (s["bvh_builder"], 0)
    s["bvh_kind"] = kind
    return s


def camera(origin, target, up, fov_deg, width, height, near=0.1, far=100.0):
    """(c2w, s2c) as the reference computes them: window.cpp:230-233 with modelM = I (scene.cpp:93,113)."""
    view = host.look_at(origin, target, up)
    proj = host.perspective(float(fov_deg), float(width) / float(height), near, far)
    return host.mat4_inverse(view), host.mat4_inverse(proj)


def make_params(c2w, s2c, width, height, max_depth, n_samples=1, seed=(0.137, 0.731), aperture=0.0, focal=1.0):
    return dict(c2w=np.asarray(c2w, np.float32), s2c=np.asarray(s2c, np.float32), width=int(width),
                height=int(height), max_depth=int(max_depth), n_samples=int(n_samples),
                seed=(float(np.float32(seed[0])), float(np.float32(seed[1]))), aperture=float(aperture),
                focal=float(focal))


def box(lo, hi):
    """Closed axis-aligned box, 12 triangles with flat OUTWARD normals: a media box is entered through a face seen from the front
    (the volume branch, raytrace.frag:424) and its trial rays end on the inside of the opposite face."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    d = hi - lo
    X, Y, Z = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    faces = [quad(lo, Y, X), quad(lo + Z, X, Y),          # -z, +z
             quad(lo, X, Z), quad(lo + Y, Z, X),          # -y, +y
             quad(lo, Z, Y), quad(lo + X, Y, Z)]          # -x, +x
    return np.concatenate([f[0] for f in faces], 0), np.concatenate([f[1] for f in faces], 0)


# --------------------------------------------------------------------------- volumes (GLRTX_EXT_VOLUME)
def fire_grids(n=(16, 16, 16), temperature=10.0, seed=0):
    """A smooth blob: density and temperature fall off from a centre low in the box, with a little deterministic noise.
    Returns (density, temperature) float32 grids shaped (nz, ny, nx), x fastest."""
    nx, ny, nz = n
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    r2 = ((x - 0.5) / 0.35) ** 2 + ((y - 0.35) / 0.45) ** 2 + ((z - 0.5) / 0.35) ** 2
    rng = np.random.default_rng(seed)
    dens = np.clip(1.0 - r2, 0.0, None) * (0.8 + 0.4 * rng.random((nz, ny, nx)))
    temp = temperature * np.clip(1.0 - 0.8 * r2, 0.0, None)
    return dens.astype(np.float32), temp.astype(np.float32)


def config_fire(width=1920, height=1080, max_depth=8, n_samples=1, grid=64, temperature=10.0, bvh="sah"):
    """A media box holding a fire blob (grid^3 voxels) over a diffuse floor, a lamp above.  Returns (scene, params, volume) with
    volume = dict(density, temperature, bbox_min, bbox_max) for Device.upload_volume."""
    b = SceneBuilder()
    fog = b.add_material(media())
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    lamp = b.add_material(emitter((6.0, 6.0, 6.0)))
    lo, hi = (-1.0, 0.05, -1.0), (1.0, 2.05, 1.0)
    b.add_mesh(*box(lo, hi), fog)
    b.add_mesh(*quad((-6, 0, 6), (12, 0, 0), (0, 0, -12)), grey)
    b.add_mesh(*quad((-1, 4, -1), (2, 0, 0), (0, 0, 2)), lamp)  # normal -y
    scene = b.build(bvh)
    dens, temp = fire_grids((grid, grid, grid), temperature)
    c2w, s2c = camera((0, 2.2, 6), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples), dict(density=dens, temperature=temp, bbox_min=lo, bbox_max=hi)


def write_vol(path, grid, bbox_min=(0.0, 0.0, 0.0), bbox_max=(1.0, 1.0, 1.0)):
    """A Mitsuba-style VOL grid file, version 3: "VOL" 3, int32 encoding 1 (float32), int32 xres yres zres channels, six float32
    bbox values (min xyz, max xyz), then float32 data, channels fastest, then x, y, z.  grid: (nz, ny, nx) or (nz, ny, nx, channels)."""
    g = np.asarray(grid, np.float32)
    if g.ndim == 3:
        g = g[..., None]
    nz, ny, nx, nc = g.shape
    hdr = b"VOL\x03" + np.array([1, nx, ny, nz, nc], "<i4").tobytes() + np.array([*bbox_min, *bbox_max], "<f4").tobytes()
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(np.ascontiguousarray(g, "<f4").tobytes())


def read_vol(path):
    """Inverse of write_vol: (grid (nz, ny, nx, channels) float32, bbox_min, bbox_max).  Rejects anything but version 3 float32."""
    raw = open(path, "rb").read()
    if len(raw) < 48 or raw[:3] != b"VOL":
        raise ValueError(f"{path}: not a VOL file")
    if raw[3] != 3:
        raise ValueError(f"{path}: VOL version {raw[3]}, only 3 is supported")
    enc, nx, ny, nz, nc = np.frombuffer(raw, "<i4", 5, 4)
    if enc != 1:
        raise ValueError(f"{path}: VOL encoding {enc}, only 1 (float32) is supported")
    bb = np.frombuffer(raw, "<f4", 6, 24)
    n = int(nx) * int(ny) * int(nz) * int(nc)
    if nx <= 0 or ny <= 0 or nz <= 0 or nc <= 0 or len(raw) < 48 + 4 * n:
        raise ValueError(f"{path}: VOL header {nx}x{ny}x{nz}x{nc} does not match the file size {len(raw)}")
    g = np.frombuffer(raw, "<f4", n, 48).reshape(int(nz), int(ny), int(nx), int(nc)).astype(np.float32)
    return g, tuple(float(v) for v in bb[:3]), tuple(float(v) for v in bb[3:])


def write_ppm(path, rgb):
    """A binary PPM (P6, 8-bit) of rgb (height, width, 3) uint8 whose ROW 0 IS t = 0: the file's rows run from the top of the picture down, so they are
    written last row first (the top row of a PPM is t = 1, OBJ's convention)."""
    a = np.ascontiguousarray(rgb, np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(a[::-1].tobytes())


def write_pfm(path, rgb):
    """A little-endian PFM ("PF", scale -1) of rgb (height, width, 3) float32 whose row 0 is t = 0: a PFM's rows run from the bottom up, as the array's do."""
    a = np.ascontiguousarray(rgb, "<f4")
    assert a.ndim == 3 and a.shape[2] == 3
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())


def volume_from_file_grid(grid):
    """What the reference uploads from a VOL grid (scene.cpp:183-188): glTexSubImage3D with GL_RED reads the FIRST nx*ny*nz floats of
    the data, whatever the channel count; u_densityMax is the maximum over all of it.  Returns (grid (nz, ny, nx), max)."""
    g = np.asarray(grid, np.float32)
    nz, ny, nx = g.shape[:3]
    return g.reshape(-1)[: nx * ny * nz].reshape(nz, ny, nx).copy(), float(g.max())


COPPER = dict(eta=(0.200, 0.924, 1.102), kappa=(3.912, 2.452, 2.142))


# --------------------------------------------------------------------------- BASELINE configs
def config_c1(width=256, height=256, max_depth=1, n_samples=1, bvh="sah", subdiv=2):
    """3 icospheres + ground quad + emitter quad; 964 triangles at subdiv 2."""
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    red = b.add_material(diffuse((0.8, 0.3, 0.3)))
    cu = b.add_material(conductor(COPPER["eta"], COPPER["kappa"], 0.2))
    lamp = b.add_material(emitter((10.0, 10.0, 10.0)))
    b.add_mesh(*quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)  # normal +y
    b.add_mesh(*icosphere(subdiv, 1.0, (-2.2, 1.0, 0.0)), red)
    b.add_mesh(*icosphere(subdiv, 1.0, (0.0, 1.0, 0.0)), cu)
    b.add_mesh(*icosphere(subdiv, 1.0, (2.2, 1.0, 0.0)), grey)
    b.add_mesh(*quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)  # normal -y
    scene = b.build(bvh)
    c2w, s2c = camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples)


def dielectric(ior, tint=(1.0, 1.0, 1.0)):
    """EXTENSION material (no reference counterpart: MTRL_DIELECTRIC = 4 is declared at raytrace.frag:32 and never branched on, so
    without GLRTX_EXT_DIELECTRIC it renders black, like in the reference): param0 = tint, param1.x = index of refraction."""
    return dict(type=4, param0=tint, param1=(float(ior), 0.0, 0.0))


def config_spheres(width=256, height=256, max_depth=4, n_samples=1, subdiv=None, glass=False, bvh="sah"):
    """BASELINE configs[0] read literally -- "3 spheres + 1 ground plane": the C1 layout with the three spheres ANALYTIC
    (subdiv None; returned as a third value, (n, 5) rows [cx, cy, cz, radius, material] for glrtx_upload_spheres) or, for the
    tessellation-limit comparison, as icospheres of the given subdivision on the pinned triangle path (third value None).
    glass: the middle sphere is a dielectric (ior 1.5) instead of copper.  PARITY UNPINNED (no spheres in the reference)."""
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    red = b.add_material(diffuse((0.8, 0.3, 0.3)))
    mid = b.add_material(dielectric(1.5) if glass else conductor(COPPER["eta"], COPPER["kappa"], 0.2))
    lamp = b.add_material(emitter((10.0, 10.0, 10.0)))
    b.add_mesh(*quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    balls = [((-2.2, 1.0, 0.0), red), ((0.0, 1.0, 0.0), mid), ((2.2, 1.0, 0.0), grey)]
    spheres = None
    if subdiv is None:
        spheres = np.array([[c[0], c[1], c[2], 1.0, m] for c, m in balls], np.float32)
    else:
        for c, m in balls:
            b.add_mesh(*icosphere(subdiv, 1.0, c), m)
    scene = b.build(bvh)
    c2w, s2c = camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples), spheres


def config_textured_wall(n=6, width=64, height=48, max_depth=4, n_samples=2, albedo=None, per_cell=False, uv=None, seed=1, bvh="sah", texture=None):
    """A vertical wall of n x n cells (two triangles each) facing the camera behind an icosphere(1) conductor, over a grey floor and under c1's lamp: the scene
    textures are pinned on (include/glrtx.h "Textures").  A wall, not a floor: the reference's light-sampling acceptance rule leaves a surface
    parallel to the lamp nearly dark, and a dark surface shows no albedo.
      per_cell False  the wall has ONE diffuse material (param0 0.5 grey, which a bound texture replaces) and texture coordinates: `uv` (2 n n, 3, 2), by
                      default each cell's centre ((i + 0.5) / n, (j + 0.5) / n) at all three corners of its triangles -- cell (column i, row j) then reads
                      texel [j, i] of an n x n texture, or the block [2j : 2j + 2, 2i : 2i + 2] of a 2n x 2n one at the block's centre;
      per_cell True   no coordinates, and one diffuse material a cell with param0 = albedo[j, i]: what a texture constant over each cell must render as.
    The two forms have the same triangles in the same order, so the same tree.  albedo: (n, n, 3) float32, random in [0.1, 0.9] from `seed` by default.
    texture: the "texture" block export_json_obj writes for the wall's shape (scenes.diffuse).  Its materials follow its shapes' order, as Scene::parse numbers them.
    Returns (scene, params, wall) with wall = dict(n, albedo, material (the wall's id, or the first cell's), tri (its triangle range), vert (its vertex range),
    builder (the SceneBuilder, for export_json_obj), camera (export_json_obj's origin, target, up, fov))."""
    rng = np.random.default_rng(seed)
    alb = np.asarray(rng.uniform(0.1, 0.9, (n, n, 3)) if albedo is None else albedo, np.float32).reshape(n, n, 3)
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    cu = b.add_material(conductor(COPPER["eta"], COPPER["kappa"], 0.2))
    lamp = b.add_material(emitter((10.0, 10.0, 10.0)))
    b.add_mesh(*quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*icosphere(1, 1.0, (0.0, 1.0, 0.0)), cu)
    b.add_mesh(*quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    first_tri = sum(p.shape[0] for p in b._pos)
    x0, y0, z0, w, h = -5.0, 0.0, -2.0, 10.0, 6.0
    pos, nrm, mid, st = [], [], [], []
    wall = len(b.materials) if per_cell else b.add_material(diffuse((0.5, 0.5, 0.5), texture))
    for j in range(n):
        for i in range(n):
            p, q = quad((x0 + w * i / n, y0 + h * j / n, z0), (w / n, 0, 0), (0, h / n, 0))  # normal +z, towards the camera
            pos.append(p); nrm.append(q)
            mid += [b.add_material(diffuse(tuple(float(c) for c in alb[j, i]))) if per_cell else wall] * 2
            st.append(np.broadcast_to(np.array([(i + 0.5) / n, (j + 0.5) / n], np.float32), (2, 3, 2)))
    coords = None if per_cell else (np.concatenate(st, 0) if uv is None else uv)
    b.add_mesh(np.concatenate(pos, 0), np.concatenate(nrm, 0), np.asarray(mid, np.float32), uv=coords)
    scene = b.build(bvh)
    c2w, s2c = camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    info = dict(n=n, albedo=alb, material=wall, tri=range(first_tri, first_tri + 2 * n * n), vert=range(3 * first_tri, 3 * (first_tri + 2 * n * n)), builder=b,
                camera=((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0))
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples), info


def config_mapped_wall(n=6, width=64, height=48, max_depth=4, n_samples=2, wall="conductor", alpha=None, per_cell=False, uv="cell", seed=1, bvh="sah",
                       normal_map=None, roughness_map=None, lamp=10.0):
    """config_textured_wall's scene with a CONDUCTOR (copper) or DIFFUSE wall material: the scene material maps are pinned on (include/glrtx.h "Material maps").
      per_cell False  the wall has ONE material (conductor: alpha 0.2) and texture coordinates.  uv "cell": each cell's centre ((i + 0.5) / n, (j + 0.5) / n) at
                      all three corners -- a roughness map is then constant over a cell, and a normal map finds det = 0 and keeps the normal; uv "corner": the
                      wall's own parametrisation, s = x across, t = y up, in [0, 1] -- what a normal map needs; or an array (2 n n, 3, 2).
      per_cell True   (conductor only) no coordinates, and one conductor material a cell with param2 = (alpha[j, i, 0], alpha[j, i, 1], 0): what a roughness map
                      constant over each cell must render as.
    The forms have the same triangles in the same order, so the same tree.  alpha: (n, n, 2) float32, random in [0.05, 0.5] from `seed` by default.
    normal_map / roughness_map: the blocks export_json_obj writes for the wall's shape.  Returns (scene, params, wall) as config_textured_wall does, with
    wall["alpha"] in place of the albedo."""
    if wall not in ("conductor", "diffuse") or (per_cell and wall != "conductor"):
        raise ValueError("config_mapped_wall: wall is 'conductor' or 'diffuse'; per_cell needs the conductor")
    rng = np.random.default_rng(seed)
    al = np.asarray(rng.uniform(0.05, 0.5, (n, n, 2)) if alpha is None else alpha, np.float32).reshape(n, n, 2)
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    cu = b.add_material(conductor(COPPER["eta"], COPPER["kappa"], 0.2))
    lamp_id = b.add_material(emitter((lamp, lamp, lamp)))
    b.add_mesh(*quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*icosphere(1, 1.0, (0.0, 1.0, 0.0)), cu)
    b.add_mesh(*quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp_id)
    first_tri = sum(p.shape[0] for p in b._pos)
    x0, y0, z0, w, h = -5.0, 0.0, -2.0, 10.0, 6.0

    def cell_material(ax, ay):
        m = conductor(COPPER["eta"], COPPER["kappa"], 0.2)
        m["param2"] = (float(ax), float(ay), 0.0)
        return m

    one = diffuse((0.5, 0.5, 0.5)) if wall == "diffuse" else conductor(COPPER["eta"], COPPER["kappa"], 0.2)
    for key, block in (("normal_map", normal_map), ("roughness_map", roughness_map)):
        if block is not None:
            one[key] = block
    wall_id = len(b.materials) if per_cell else b.add_material(one)
    pos, nrm, mid, st = [], [], [], []
    for j in range(n):
        for i in range(n):
            p, q = quad((x0 + w * i / n, y0 + h * j / n, z0), (w / n, 0, 0), (0, h / n, 0))  # normal +z, towards the camera
            pos.append(p); nrm.append(q)
            mid += [b.add_material(cell_material(*al[j, i])) if per_cell else wall_id] * 2
            if isinstance(uv, str) and uv == "corner":
                c = np.array([[i, j], [i + 1, j], [i + 1, j + 1], [i, j + 1]], np.float32) / np.float32(n)
                st.append(np.stack([c[[0, 1, 2]], c[[0, 2, 3]]]))  # quad(): triangles (a, b, c), (a, c, d)
            else:
                st.append(np.broadcast_to(np.array([(i + 0.5) / n, (j + 0.5) / n], np.float32), (2, 3, 2)))
    coords = None if per_cell else (np.concatenate(st, 0) if isinstance(uv, str) else uv)
    b.add_mesh(np.concatenate(pos, 0), np.concatenate(nrm, 0), np.asarray(mid, np.float32), uv=coords)
    scene = b.build(bvh)
    c2w, s2c = camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    info = dict(n=n, alpha=al, material=wall_id, tri=range(first_tri, first_tri + 2 * n * n), vert=range(3 * first_tri, 3 * (first_tri + 2 * n * n)), builder=b,
                camera=((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0))
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples), info


def collapse_triangles(scene, tris):
    """The scene with vertices 1 and 2 of each wire triangle in `tris` moved onto its vertex 0 (positions only; the triangles' vertices must be unshared, as
    SceneBuilder makes them) and every other buffer -- the `bvh` array included -- as it is.  A collapsed triangle has det = 0 and is never hit, and the tree
    still encloses it: the image is the one a traversal that rejects every candidate on those triangles renders (include/glrtx.h "Cutouts")."""
    s = dict(scene)
    v = np.array(scene["vert"], np.float32).reshape(-1, 5, 3)
    t = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    for k in np.asarray(list(tris), np.int64):
        a, b, c = (int(x) for x in t[k, :3])
        v[b, 0] = v[a, 0]
        v[c, 0] = v[a, 0]
    s["vert"] = v.reshape(-1, 3)
    return s


def config_cutout_wall(n=6, cutout=None, **kw):
    """config_textured_wall's scene as the scene alpha cutouts are pinned on (include/glrtx.h "Cutouts"): the wall's 2 n n triangles have unshared vertices and
    the cell's centre as their coordinates, so a cutout texture with one texel a cell cuts whole cells.  Returns (scene, params, wall) as config_textured_wall
    does, with two more entries: wall["cell_tris"](mask) -- the wire triangles of the cells where mask (n, n), indexed [row j, column i] as the texels are, is
    true -- and wall["collapsed"](tris, moved=None) -- collapse_triangles on the scene (or on `moved`, a moved copy of it): what the reference must be given.
    cutout: the "cutout" block export_json_obj writes for the wall's shape."""
    scene, params, wall = config_textured_wall(n=n, **kw)
    if cutout is not None:
        wall["builder"].materials[wall["material"]]["cutout"] = cutout
    first = wall["tri"][0]

    def cell_tris(mask):
        m = np.asarray(mask, bool).reshape(n, n)
        return [first + 2 * (j * n + i) + k for j in range(n) for i in range(n) if m[j, i] for k in (0, 1)]

    wall["cell_tris"] = cell_tris
    wall["collapsed"] = lambda tris, moved=None: collapse_triangles(scene if moved is None else moved, tris)
    return scene, params, wall


def config_emissive_wall(n=6, per_cell=False, emission=(4.0, 3.0, 2.0), texel=None, uv="cell", ball="conductor", width=64, height=48, max_depth=4, n_samples=2, seed=1,
                         bvh="sah", emission_map=None):
    """config_textured_wall's scene with the wall as an EMITTER panel in the light table: the scene emission maps are pinned on (include/glrtx.h "Emission
    maps").  The lamp stays, so the light table holds 2 + 2 n n triangles.
      per_cell False  the wall has ONE emitter material of `emission` and texture coordinates: uv "cell", each cell's centre at all three corners; uv "corner",
                      the wall's own parametrisation (s across, t up, in [0, 1]); or an array (2 n n, 3, 2).
      per_cell True   no coordinates, and one emitter material a cell with emission = float32(emission * texel[j, i]): what an emission map that is constant
                      over each cell, with the lookup's value texel[j, i], must render as.
    Both forms use the same triangles in the same order, and the same triangles are lights, so the tree and the light table's order are the same.
    texel: (n, n, 3) float32, random in [0.1, 0.9] from `seed` by default (never 0: a black cell would leave the light table).  ball: "conductor" (copper) or
    "glass" (a dielectric icosphere in front of the panel, for GLRTX_EXT_DIELECTRIC).  emission_map: the block export_json_obj writes for the wall's shape.
    Returns (scene, params, wall) as config_textured_wall does, with wall["texel"] and wall["emission"] in place of the albedo."""
    if ball not in ("conductor", "glass"):
        raise ValueError("config_emissive_wall: ball is 'conductor' or 'glass'")
    rng = np.random.default_rng(seed)
    c = np.asarray(rng.uniform(0.1, 0.9, (n, n, 3)) if texel is None else texel, np.float32).reshape(n, n, 3)
    e = np.broadcast_to(np.asarray(emission, np.float32), (3,)).copy()
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    mid_ball = b.add_material(dielectric(1.5) if ball == "glass" else conductor(COPPER["eta"], COPPER["kappa"], 0.2))
    lamp = b.add_material(emitter((10.0, 10.0, 10.0)))
    b.add_mesh(*quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*icosphere(1, 1.0, (0.0, 1.0, 0.0)), mid_ball)
    b.add_mesh(*quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    first_tri = sum(p.shape[0] for p in b._pos)
    x0, y0, z0, w, h = -5.0, 0.0, -2.0, 10.0, 6.0
    one = emitter(tuple(float(x) for x in e))
    if emission_map is not None:
        one["emission_map"] = emission_map
    wall_id = len(b.materials) if per_cell else b.add_material(one)
    pos, nrm, mid, st = [], [], [], []
    for j in range(n):
        for i in range(n):
            p, q = quad((x0 + w * i / n, y0 + h * j / n, z0), (w / n, 0, 0), (0, h / n, 0))  # normal +z, towards the camera
            pos.append(p); nrm.append(q)
            mid += [b.add_material(emitter(tuple(float(x) for x in (e * c[j, i]).astype(np.float32)))) if per_cell else wall_id] * 2
            if isinstance(uv, str) and uv == "corner":
                k = np.array([[i, j], [i + 1, j], [i + 1, j + 1], [i, j + 1]], np.float32) / np.float32(n)
                st.append(np.stack([k[[0, 1, 2]], k[[0, 2, 3]]]))  # quad(): triangles (a, b, c), (a, c, d)
            else:
                st.append(np.broadcast_to(np.array([(i + 0.5) / n, (j + 0.5) / n], np.float32), (2, 3, 2)))
    coords = None if per_cell else (np.concatenate(st, 0) if isinstance(uv, str) else uv)
    b.add_mesh(np.concatenate(pos, 0), np.concatenate(nrm, 0), np.asarray(mid, np.float32), uv=coords)
    scene = b.build(bvh)
    c2w, s2c = camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    info = dict(n=n, texel=c, emission=e, material=wall_id, tri=range(first_tri, first_tri + 2 * n * n), vert=range(3 * first_tri, 3 * (first_tri + 2 * n * n)),
                builder=b, camera=((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0))
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples), info


def config_emissive_panel(split=False, emission=(6.0, 6.0, 6.0), left=1.0, right=0.1, width=64, height=48, max_depth=4, n_samples=1, bvh="sah"):
    """A grey floor lit by ONE vertical emitter panel behind it and nothing else: the scene that shows that an emission map varying INSIDE a light triangle is
    sampled where it is bright (include/glrtx.h "Emission maps").
      split False  the panel is one quad with corner coordinates (s across, in [0, 1]); under a 2 x 1 nearest texture {left, right} its left half emits
                   emission * left and its right half emission * right.
      split True   the same panel as two quads, each with one emitter material of that constant emission.
    The two are not bit-comparable (other triangles, another tree); their floor irradiance has the same expectation.  Returns (scene, params, panel) with
    panel = dict(material (the panel's, or the left half's), floor (the floor's material id: plane A of the feature pass says which pixels see it))."""
    e = np.broadcast_to(np.asarray(emission, np.float32), (3,)).copy()
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    b.add_mesh(*quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    x0, y0, z0, w, h = -4.0, 0.5, -2.0, 8.0, 3.0
    if split:
        ml = b.add_material(emitter(tuple(float(x) for x in (e * np.float32(left)).astype(np.float32))))
        mr = b.add_material(emitter(tuple(float(x) for x in (e * np.float32(right)).astype(np.float32))))
        b.add_mesh(*quad((x0, y0, z0), (w / 2, 0, 0), (0, h, 0)), ml)
        b.add_mesh(*quad((x0 + w / 2, y0, z0), (w / 2, 0, 0), (0, h, 0)), mr)
    else:
        ml = b.add_material(emitter(tuple(float(x) for x in e)))
        k = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
        b.add_mesh(*quad((x0, y0, z0), (w, 0, 0), (0, h, 0)), ml, uv=np.stack([k[[0, 1, 2]], k[[0, 2, 3]]]))
    scene = b.build(bvh)
    c2w, s2c = camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples), dict(material=ml, floor=grey, builder=b, camera=((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0))


# --------------------------------------------------------------------------- environment lighting (include/glrtx.h "Environment"; PARITY UNPINNED)
ENV_QUAD_ALBEDO = (0.5, 0.25, 0.75)


def config_env_quad(width=64, height=48, max_depth=2, n_samples=16):
    """One large diffuse quad (ENV_QUAD_ALBEDO) facing +y that fills the view of a camera looking straight down, and no lights: under a constant environment E
    every pixel is albedo * E (the furnace), under any environment its mean is (albedo / pi) * the cosine-weighted integral of the upper hemisphere."""
    b = SceneBuilder()
    b.add_mesh(*quad((-50, 0, 50), (100, 0, 0), (0, 0, -100)), b.add_material(diffuse(ENV_QUAD_ALBEDO)))
    scene = b.build()
    c2w, s2c = camera((0, 5, 0), (0, 0, 0), (0, 0, -1), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples)


def config_env_sky(direction, up=None, width=64, height=48, fov_deg=10.0, max_depth=1, n_samples=1):
    """Nothing in view: a camera at the origin looking along `direction` with a narrow field of view, and a single far-away triangle behind it (a scene needs
    one).  Every pixel shows the environment."""
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    if up is None:
        up = (0.0, 0.0, -1.0) if abs(d[1]) > 0.9 else (0.0, 1.0, 0.0)
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.5, 0.5, 0.5)))
    c = -1000.0 * d
    e1 = np.cross(d, np.asarray(up, np.float64))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    pos = np.array([[c, c + e1, c + e2]], np.float32)
    b.add_mesh(pos, np.broadcast_to(d.astype(np.float32), (1, 3, 3)), grey)
    scene = b.build()
    c2w, s2c = camera((0, 0, 0), tuple(d), up, fov_deg, width, height, near=0.1, far=100.0)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples)


def config_env_box(width=64, height=48, max_depth=4, n_samples=2):
    """A closed room with a lamp under its ceiling, a conductor ball and the camera inside: no ray leaves it, whatever environment is bound."""
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    red = b.add_material(diffuse((0.8, 0.3, 0.3)))
    cu = b.add_material(conductor(COPPER["eta"], COPPER["kappa"], 0.2))
    lamp = b.add_material(emitter((10.0, 10.0, 10.0)))
    pos, nrm = box((-4, 0, -4), (4, 6, 10))
    b.add_mesh(pos, -nrm, grey)  # the walls face inward
    b.add_mesh(*icosphere(1, 1.0, (-1.5, 1.0, 0.0)), red)
    b.add_mesh(*icosphere(1, 1.0, (1.5, 1.0, 0.0)), cu)
    b.add_mesh(*quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    scene = b.build()
    c2w, s2c = camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples)


def env_octant_map():
    """A 4 x 4 float map with sixteen distinct colours (nearest filtering): the four inner texels are the upper octants, the four corners the lower ones, and an
    edge texel is shared by the upper and the lower octant of its quadrant.  Returns (4, 4, 3) float32, texel [y, x]."""
    k = np.arange(16, dtype=np.float32).reshape(4, 4)
    return np.stack([0.125 + k / 16.0, 1.0 - k / 32.0, 0.25 + (k % 4) / 8.0], -1).astype(np.float32)


def _eight_spheres(b: SceneBuilder, subdiv: int):
    xs = (-3.3, -1.1, 1.1, 3.3)
    albedos = ((0.75, 0.75, 0.75), (0.8, 0.3, 0.3), (0.3, 0.7, 0.35), (0.3, 0.4, 0.8))
    for x, a in zip(xs, albedos):
        b.add_mesh(*icosphere(subdiv, 1.0, (x, 1.0, 1.5)), b.add_material(diffuse(a)))
    for x, alpha in zip(xs, (0.05, 0.1, 0.2, 0.4)):
        b.add_mesh(*icosphere(subdiv, 1.0, (x, 3.0, -1.8)),
                   b.add_material(conductor(COPPER["eta"], COPPER["kappa"], alpha)))


def config_c2(width=1920, height=1080, max_depth=4, n_samples=1, bvh="sah", subdiv=3):
    """Cornell-style box (5 quads) + 8 icospheres + ceiling emitter; 10,252 triangles at subdiv 3."""
    b = SceneBuilder()
    white = b.add_material(diffuse((0.75, 0.75, 0.75)))
    red = b.add_material(diffuse((0.75, 0.25, 0.25)))
    green = b.add_material(diffuse((0.25, 0.75, 0.25)))
    lamp = b.add_material(emitter((15.0, 15.0, 15.0)))
    b.add_mesh(*quad((-5, 0, 5), (10, 0, 0), (0, 0, -10)), white)    # floor, +y
    b.add_mesh(*quad((-5, 10, -5), (10, 0, 0), (0, 0, 10)), white)   # ceiling, -y
    b.add_mesh(*quad((-5, 0, -5), (10, 0, 0), (0, 10, 0)), white)    # back, +z
    b.add_mesh(*quad((-5, 0, 5), (0, 0, -10), (0, 10, 0)), red)      # left, +x
    b.add_mesh(*quad((5, 0, -5), (0, 0, 10), (0, 10, 0)), green)     # right, -x
    _eight_spheres(b, subdiv)
    b.add_mesh(*quad((-2, 9.99, -2), (4, 0, 0), (0, 0, 4)), lamp)    # -y
    scene = b.build(bvh)
    c2w, s2c = camera((0, 5, 16), (0, 4.2, 0), (0, 1, 0), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples)


def config_headline(width=1920, height=1080, n_samples=1, bvh="sah", subdiv=3):
    """BASELINE.json metric: the C2 scene at 1920x1080, 8 bounces (u_maxDepth = 8)."""
    return config_c2(width, height, 8, n_samples, bvh, subdiv)


def _random_tri_scene(n, seed, extent, cam_z, width, height, max_depth, n_samples, bvh):
    pos, nrm, rng = random_triangles(n, seed, extent)
    b = SceneBuilder()
    palette = [b.add_material(diffuse(tuple(rng.uniform(0.2, 0.9, 3)))) for _ in range(64)]
    lamp = b.add_material(emitter((2.0, 2.0, 2.0)))
    is_light = rng.uniform(0.0, 1.0, n) < 0.2
    mid = np.where(is_light, lamp, np.asarray(palette)[rng.integers(0, 64, n)])
    b.add_mesh(pos, nrm, mid)
    scene = b.build(bvh)
    c2w, s2c = camera((0, 0, cam_z), (0, 0, 0), (0, 1, 0), 40.0, width, height, 0.1, 200.0)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples)


def config_c3(width=1920, height=1080, max_depth=1, n_samples=1, bvh="chain", n=10_000):
    """10k random triangles; bvh='chain' is the brute-force linear scan, 'sah' the same scene with a real tree."""
    return _random_tri_scene(n, 20260101, 4.0, 14.0, width, height, max_depth, n_samples, bvh)


def config_c4(width=3840, height=2160, max_depth=8, n_samples=16, bvh="sah", subdiv=3):
    """8 icospheres + ground + emitter (no box)."""
    b = SceneBuilder()
    grey = b.add_material(diffuse((0.7, 0.7, 0.7)))
    lamp = b.add_material(emitter((12.0, 12.0, 12.0)))
    b.add_mesh(*quad((-15, 0, 15), (30, 0, 0), (0, 0, -30)), grey)
    _eight_spheres(b, subdiv)
    b.add_mesh(*quad((-3, 9.0, -3), (6, 0, 0), (0, 0, 6)), lamp)
    scene = b.build(bvh)
    c2w, s2c = camera((0, 5, 16), (0, 2.0, 0), (0, 1, 0), 40.0, width, height)
    return scene, make_params(c2w, s2c, width, height, max_depth, n_samples)


def config_c5(width=1920, height=1080, max_depth=4, n_samples=1, bvh="sah", n=100_000):
    return _random_tri_scene(n, 20260102, 10.0, 34.0, width, height, max_depth, n_samples, bvh)


CONFIGS = {"c1": config_c1, "c2": config_c2, "c3": config_c3, "c4": config_c4, "c5": config_c5,
           "headline": config_headline}


def scene_bytes(scene) -> int:
    """Algorithmic bytes of one read of the compact scene: 72 B/triangle (3 pos + 3 normals),
    16 B/triangle (indices + material), 36 B/node, 72 B/material, 16 B/light."""
    n_tri = scene["tri"].reshape(-1, 4).shape[0]
    n_node = scene["bvh"].reshape(-1, 9).shape[0]
    n_mat = scene["mat"].reshape(-1, 18).shape[0]
    n_light = scene["light"].reshape(-1, 4).shape[0]
    return 88 * n_tri + 36 * n_node + 72 * n_mat + 16 * n_light


# --------------------------------------------------------------------------- JSON + OBJ export (Scene::parse input)
def export_json_obj(builder: SceneBuilder, directory, width, height, origin, target, up, fov_deg, near=0.1, far=100.0,
                    aperture=None, focal=None, name="scene.json"):
    """Write `builder`'s meshes as one OBJ per add_mesh() call plus the JSON scene description the
    reference's Scene::parse reads (schema: SURVEY.md Appendix C).  Floats are written with 9 significant
    digits, which round-trips float32 exactly.  Returns the JSON path."""
    import json
    import pathlib

    d = pathlib.Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    shapes = []
    for k, (pos, nrm, mid, uv) in enumerate(zip(builder._pos, builder._nrm, builder._mid, builder._uv)):
        assert np.all(mid == mid[0]), "one material per shape (scene.cpp:124-219)"
        m = builder.materials[int(mid[0])]
        lines = []
        for p in pos.reshape(-1, 3):
            lines.append("v %.9g %.9g %.9g" % tuple(p))
        for n in nrm.reshape(-1, 3):
            lines.append("vn %.9g %.9g %.9g" % tuple(n))
        if uv is not None:  # (a mesh added with texture coordinates: vt lines and v/vt/vn corners)
            for c in uv.reshape(-1, 2):
                lines.append("vt %.9g %.9g" % tuple(c))
        for t in range(pos.shape[0]):
            a = 3 * t + 1
            lines.append(f"f {a}/{a}/{a} {a + 1}/{a + 1}/{a + 1} {a + 2}/{a + 2}/{a + 2}" if uv is not None else f"f {a}//{a} {a + 1}//{a + 1} {a + 2}//{a + 2}")
        (d / f"shape{k}.obj").write_text("\n".join(lines) + "\n")
        sh = {"type": "obj", "filename": f"shape{k}.obj"}
        if m["type"] == MTRL_DIFFUSE:
            sh.update(material="diffuse", reflectance=[float(v) for v in m["param0"]])
            if m.get("texture") is not None:
                sh["texture"] = dict(m["texture"]) if isinstance(m["texture"], dict) else m["texture"]
        elif m["type"] == MTRL_CONDUCTOR:
            sh.update(material="conductor", kappa=[float(v) for v in m["param0"]], eta=[float(v) for v in m["param1"]],
                      alpha=float(m["param2"][0]))
        elif m["type"] == MTRL_EMITTER:
            sh.update(material="emitter", emission=[float(v) for v in m["emission"]])
            if m.get("emission_map") is not None:  # (config_emissive_wall; host/scene.h: emissionMapSpecs)
                sh["emission_map"] = dict(m["emission_map"])
        elif m["type"] == MTRL_MEDIA:
            sh.update(material="media")
            if m.get("volume") is not None:
                sh["volume"] = {k: (v if isinstance(v, str) else [float(c) for c in v]) for k, v in m["volume"].items()}
        else:
            raise ValueError("export supports diffuse / conductor / emitter / media shapes")
        for key in ("normal_map", "roughness_map", "cutout"):  # (config_mapped_wall, config_cutout_wall; host/scene.h: MapSpec, CutoutSpec)
            if m.get(key) is not None:
                sh[key] = dict(m[key]) if isinstance(m[key], dict) else m[key]
        shapes.append(sh)
    cam = {"type": "perspective", "fov": fov_deg, "nearClip": near, "farClip": far,
           "lookAt": {"origin": list(origin), "target": list(target), "up": list(up)}}
    if aperture is not None:
        cam["apertureRadius"] = aperture
    if focal is not None:
        cam["focalLength"] = focal
    doc = {"film": {"width": width, "height": height}, "camera": cam, "scene": shapes}
    (d / name).write_text(json.dumps(doc, indent=1))
    return d / name
