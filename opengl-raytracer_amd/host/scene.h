// scene.h -- glrt::Scene, the drop-in scene class (reference: src/core/scene.h:45-74).
// Same public surface: Scene(), Scene(filename), parse(filename); Window reads the private state as
// a friend exactly like the reference's Window does (scene.h:73).  Where the reference held GL
// TextureBuffer objects (scene.h:63-67) this class holds the flat host buffers in the identical
// byte layout and hands them to glrtx_upload_scene (include/glrtx.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"
#include "texture_file.h"
#include "volume.h"

namespace glrt {

class Json;

// Wire-format records, byte-identical to the reference's (scene.h:16-35, trimesh.h:15-25, bvh.h:84-100).
struct Vertex { float pos[3], normal[3], uv[3], tangent[3], binormal[3]; };
struct Triangle { float indices[4]; };  // i, j, k, materialId
enum class MaterialType : int { Emitter = 1, Diffuse = 2, Conductor = 3, Dielectric = 4, Media = 5 };
struct Material { float type[3], emission[3], param0[3], param1[3], param2[3], texIds[3]; };
struct BVHNode { float bboxMin[3], bboxMax[3], children[3]; };

class GLRT_API Scene {
public:
    Scene();
    explicit Scene(const std::string &filename);
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;

    // JSON scene description (schema: SURVEY.md Appendix C, derived from scene.cpp:57-250).
    void parse(const std::string &filename);

    // Programmatic alternative to parse(): adopt already-flat buffers (synthetic scenes, tests).
    void setBuffers(int width, int height, const float viewM[16], const float projM[16], float apertureRadius,
                    float focalLength, std::vector<Vertex> vertices, std::vector<Triangle> triangles,
                    std::vector<Material> materials, std::vector<BVHNode> nodes = {});

    int filmWidth() const { return width; }
    int filmHeight() const { return height; }
    size_t numTriangles() const { return triangles.size(); }
    size_t numLights() const { return lights.size(); }
    size_t numNodes() const { return nodes.size(); }
    int bvhDepth() const { return bvhDepth_; }
    // "sah" (default) | "sah-gpu" / "lbvh" (built on the GPU) | "sah-levels-cpu" / "lbvh-cpu" | "reference" (the reference host's own tree, never re-ordered); call before parse().  GLRT_BVH overrides.
    void setBvhBuilder(const std::string &kind) { bvhBuilder_ = kind; }
    // EXTENSIONS beyond the reference (parity unpinned; include/glrtx.h).  Off, parse() is the reference's: "dielectric" is an
    // unsupported material (FatalError, scene.cpp:216-218) and a shape that is not "obj" contributes no geometry (scene.cpp:222).
    // On (call before parse(); GLRT_EXTENSIONS=1): material "dielectric" {"ior": n, "tint": [r,g,b]} and shape
    // {"type": "sphere", "center": [x,y,z], "radius": r} are accepted; Window then uploads the spheres and enables
    // GLRTX_EXT_DIELECTRIC (and GLRTX_EXT_WHITTED if setWhitted(true)).
    void enableExtensions(bool on) { extensions_ = on; }
    void setWhitted(bool on) { whitted_ = on; }
    size_t numSpheres() const { return spheres.size() / 5; }
    // Textures (include/glrtx.h "Textures"; no reference counterpart).  With extensions on, a "diffuse" shape may carry
    //     "texture": {"file": "x.ppm" | "x.pfm", "filter": "bilinear" | "nearest", "wrap": "repeat" | "clamp", "srgb": true | false}
    // "file" is required and resolved against the scene file's directory: a binary PPM (P6, 8-bit) or a PFM (float, linear), read by texture_file.h with
    // row 0 at t = 0 (the top row of a PPM is t = 1, OBJ's convention).  "filter" defaults to "bilinear", "wrap" to "repeat" (both axes), "srgb" to true; it
    // selects GLRTX_TEX_RGBA8_SRGB or _UNORM for a PPM and says nothing about a PFM.  The texture replaces "reflectance" as the shape's albedo, looked up at
    // the OBJ's vt coordinates.  An unreadable file and a value other than those above are FatalErrors that name the key.  Window uploads the set after the
    // scene (glrtx_upload_textures).  With extensions off the key is ignored, as the reference ignores keys it does not know; a file without it parses and
    // renders as before.
    struct TextureSpec {
        size_t material;  // the shape's material
        std::string file;
        int format, wrap, filter;  // GLRTX_TEX_*
        TextureImage image;
    };
    const std::vector<TextureSpec> &textureSpecs() const { return textures_; }
    // Material maps (include/glrtx.h "Material maps"; no reference counterpart).  With extensions on, a "diffuse" or "conductor" shape may carry
    //     "normal_map": {"file": "x.pfm" | "x.ppm", "filter": .., "wrap": .., "scale": x}      and a "conductor" shape
    //     "roughness_map": {"file": "x.pfm" | "x.ppm", "filter": .., "wrap": ..}
    // "file", "filter" and "wrap" as in "texture".  A PPM is read as GLRTX_TEX_RGBA8_UNORM: a map holds vectors, not colours, and "srgb": true is a
    // FatalError.  "scale" (normal maps; default 1) is the normal map's scale and must be finite.  Both are looked up at the OBJ's vt coordinates.  A map on a
    // shape of another material and a value other than those above are FatalErrors that name the key.  Window uploads the maps' images behind the textures in
    // the one set and binds them (glrtx_bind_material_maps).  With extensions off the keys are ignored, as "texture" is.
    struct MapSpec {
        size_t material;  // the shape's material
        bool roughness;   // false: a normal map
        std::string file;
        int format, wrap, filter;  // GLRTX_TEX_*
        float scale;
        TextureImage image;
    };
    const std::vector<MapSpec> &mapSpecs() const { return maps_; }
    // Cutouts (include/glrtx.h "Cutouts"; no reference counterpart).  With extensions on, a "diffuse" or "conductor" shape may carry
    //     "cutout": {"file": "mask.ppm" | "mask.pfm", "channel": "r" | "g" | "b", "cutoff": x, "filter": .., "wrap": ..}
    // "file", "filter" and "wrap" as in "texture".  A PPM is read as GLRTX_TEX_RGBA8_UNORM: a mask holds coverage, not colour, and "srgb": true is a
    // FatalError.  "channel" defaults to "r" -- the readers are three-channel, so alpha in files is not offered: channel 3 is for callers of the C ABI --,
    // "cutoff" to 0.5 and must be finite.  The mask is looked up at the OBJ's vt coordinates; a candidate hit counts where the channel's value >= cutoff.  A
    // cutout on a shape of another material and a value other than those above are FatalErrors that name the shape and the key.  Window uploads the masks'
    // images behind the textures and maps in the one set and binds them (glrtx_bind_cutouts).  With extensions off the key is ignored, as "texture" is.
    struct CutoutSpec {
        size_t material;  // the shape's material
        std::string file;
        int format, wrap, filter;  // GLRTX_TEX_*
        int channel;               // 0 .. 2
        float cutoff;
        TextureImage image;
    };
    const std::vector<CutoutSpec> &cutoutSpecs() const { return cutouts_; }
    // Emission maps (include/glrtx.h "Emission maps"; no reference counterpart).  With extensions on, an "emitter" shape may carry
    //     "emission_map": {"file": "x.ppm" | "x.pfm", "filter": .., "wrap": .., "srgb": ..}
    // with the keys of "texture" and their defaults (a PPM is sRGB unless "srgb": false).  The map is looked up at the OBJ's vt coordinates and MULTIPLIES the
    // shape's "emission", where the emitter is seen and where next-event estimation samples it.  A value other than those above is a FatalError that names
    // the shape and the key.  Window uploads the images behind the textures, maps and masks in the one set and binds them (glrtx_bind_emission_maps); a scene
    // that carries both a "cutout" and an "emission_map" is refused there, as the device refuses it.  With extensions off the key is ignored, as "texture" is.
    const std::vector<TextureSpec> &emissionMapSpecs() const { return emissionMaps_; }
    // Environment (include/glrtx.h "Environment"; no reference counterpart).  With extensions on, the scene file may carry the top-level key
    //     "environment": {"file": "x.pfm" | "x.ppm", "layout": "latlong" | "octahedral", "size": N, "mode": "escape" | "sampled", "scale": x | [r, g, b],
    //                     "rotate_y": degrees, "light_pick": p, "filter": "bilinear" | "nearest", "srgb": true | false}
    // "file" is required and read as a texture's is (texture_file.h: row 0 is the bottom row of the picture).  "layout" defaults to "latlong": the picture --
    // +y up, its top row +y, its centre column -z -- is resampled into a size x size octahedral float map (glrt_env_from_latlong; "size" defaults to 512, 2 ..
    // 16384).  "octahedral": the file IS the map (square; row 0 at t = 0; "size" is not read) in the file's own format.  "mode" defaults to "escape", "scale"
    // to 1, "rotate_y" to 0 (a positive angle turns the map so that what it holds along +z is seen along +x after a quarter turn), "light_pick" to 0.5,
    // "filter" to "bilinear", "srgb" to true (a PPM's bytes; a PFM is linear).  A value other than those above and an unreadable file are FatalErrors that
    // name the key.  Window uploads it after the scene (glrtx_upload_environment).  glrt_main --env-mode overrides "mode" (setEnvMode, before parse()).
    // With extensions off the key is ignored, as the reference ignores keys it does not know.  Together with enableVolume(true) it is a FatalError: the volume
    // branch has its own escape path.
    struct EnvironmentSpec {
        bool present = false;
        std::string file;
        bool latlong = true;
        int size = 0, format = 0, filter = 1, mode = 0;  // the map's side; GLRTX_TEX_*; GLRTX_ENV_*
        float scale[3] = {1.0f, 1.0f, 1.0f};
        float rotateY = 0.0f, lightPick = 0.5f;
        std::vector<unsigned char> texels;  // the octahedral map, row 0 at t = 0
    };
    const EnvironmentSpec &environmentSpec() const { return environment_; }
    void setEnvMode(int mode) { envModeOverride_ = mode; }  // GLRTX_ENV_*; -1: the file's
    // Participating media (the reference's volume branch, which it compiles out: raytrace.frag:4; include/glrtx.h GLRTX_EXT_VOLUME).  parse() always keeps
    // each "media" shape's "volume" block {density, temperature, bboxMin, bboxMax} (scene.cpp:174-214) in volumeSpecs(); with enableVolume(true) (call
    // before parse()) it also reads the FIRST block's two VOL files -- a missing or unreadable file is then a FatalError -- and Window uploads them and
    // sets GLRTX_EXT_VOLUME.  Off, the files are not opened and the media surfaces pass rays through unchanged, as in the reference.
    struct VolumeSpec {
        std::string density, temperature;  // paths, resolved against the scene file's directory
        float bboxMin[3], bboxMax[3];      // from the JSON (u_bboxMin / u_bboxMax), not from the files
    };
    void enableVolume(bool on) { volume_ = on; }
    const std::vector<VolumeSpec> &volumeSpecs() const { return volumeSpecs_; }
    bool hasVolume() const { return hasVolume_; }

    // Animation (no reference counterpart; glrt_main --animate, Window::setAnimation): call after parse().  FILE is JSON,
    //     {"steps": [ {"matrices": [[shape, m0, ..., m11], ...], "camera": { ... }}, ... ]}
    // shape: an index into the scene file's "scene" array; m0 .. m11: that shape's pose matrix, row-major 3x4 (include/glrtx.h "Posing").  Shapes a step does not
    // list get the identity.  "camera" is optional and has the keys of the scene file's own "camera" block (it goes through the same code); without it the scene
    // file's camera holds for that step.  Numbers are parsed as doubles and cast to float.  A shape index out of range and an entry that is not 13 numbers are
    // FatalErrors.  Bone i of the rig Window uploads is shape i: loadObj yields three fresh vertices per triangle, so shapes never share a vertex.
    //
    // Morph targets (include/glrtx.h "Deforming").  The file may carry a top-level "targets": [{"shape": i, "file": "x.obj"}, ...] (at most 64; the path is
    // resolved against the animation file's directory) and each step "weights": [[target, w], ...]; targets a step does not list get 0.  A target OBJ goes
    // through loadObj and must give shape i's vertex count (otherwise a FatalError names both counts); its delta is target - rest for position and normal, one
    // float subtraction each, and zero outside the shape.  A file without "targets" is what it was.
    //
    // Sparse targets (include/glrtx.h "Deforming", SPARSE TARGETS).  With a top-level "sparse_targets": true the limit is 1024 targets instead of 64 and the
    // parser builds the sparse set directly from each target OBJ: a vertex of the shape gets an entry iff its delta passes glrt_morph_sparsify's rule (some
    // component with a non-zero exponent field); the dense targets x vertices x 6 array is never allocated and morphDeltas() stays empty.  Window uploads the
    // set with glrtx_upload_morph_targets_sparse.  A file without the key parses, uploads and renders as before.
    //
    // Rebuilding normals (include/glrtx.h "Rebuilding normals").  With a top-level "rebuild_normals": true Window uploads the normal topology of the scene's
    // vertices beside the rig and sets glrtx_set_pose_normals before the first step: every step's normals are rebuilt from its moved faces.  An optional
    // "weld": "positions" welds by position alone (GLRTX_NORMALS_WELD_POSITIONS); "weld": "normals" is the default's name.  Anything but true or false, and any
    // other "weld", is a FatalError naming the key.  A file without the keys renders as before.
    struct AnimationStep {
        std::vector<float> matrices;  // numShapes() x 12
        std::vector<float> weights;   // numMorphTargets()
        bool hasCamera = false;
        float viewM[16], projM[16], apertureRadius = 0.0f, focalLength = 0.0f;  // (with hasCamera)
    };
    void parseAnimation(const std::string &filename);
    const std::vector<AnimationStep> &animation() const { return animation_; }
    size_t numShapes() const { return shapeFirstVertex_.size(); }
    size_t numMorphTargets() const { return morphShape_.size(); }
    // the targets' deltas as glrtx_upload_morph_targets takes them: numMorphTargets() x vertex count x 6 floats {dpos, dnormal}
    const std::vector<float> &morphDeltas() const { return morphDeltas_; }
    // with "sparse_targets": true, the set as glrtx_upload_morph_targets_sparse takes it: offsets (numMorphTargets() + 1), vertex and deltas (6 floats an entry)
    bool morphSparse() const { return morphSparse_; }
    const std::vector<uint64_t> &morphOffsets() const { return morphOffsets_; }
    const std::vector<uint32_t> &morphVertex() const { return morphVertex_; }
    const std::vector<float> &morphSparseDeltas() const { return morphSparseDeltas_; }
    // "rebuild_normals": true, and the flags "weld" asks glrtx_upload_normal_topology for
    bool rebuildNormals() const { return rebuildNormals_; }
    unsigned normalTopologyFlags() const { return normalFlags_; }
    // the first vertex of entry i of the JSON "scene" array (an entry without geometry owns none: its range is empty); i == numShapes(): the vertex count
    size_t shapeFirstVertex(size_t i) const { return i < shapeFirstVertex_.size() ? shapeFirstVertex_[i] : vertices.size(); }

private:
    void finalize();  // lights list + BVH (scene.cpp:246-256)
    // a "camera" block of type "perspective" (scene.cpp:62-114) into the four camera fields given; the scene file's and an animation step's alike
    void readPerspective(const Json &cam, float view[16], float proj[16], float &aperture, float &focal) const;

    int width = 0, height = 0;
    float apertureRadius = 0.0f, focalLength = 1.0f;
    float modelM[16], viewM[16], projM[16];  // column-major

    std::vector<Vertex> vertices;
    std::vector<Triangle> triangles;
    std::vector<Triangle> lights;
    std::vector<Material> materials;
    std::vector<BVHNode> nodes;
    int bvhDepth_ = 0;
    std::string bvhBuilder_ = "sah";
    std::vector<float> spheres;  // extension: 5 floats per sphere {cx, cy, cz, radius, material}
    std::vector<TextureSpec> textures_;  // extension: one per textured diffuse shape, in shape order
    std::vector<MapSpec> maps_;          // extension: the shapes' normal and roughness maps, in shape order
    std::vector<CutoutSpec> cutouts_;    // extension: the shapes' cutout masks, in shape order
    std::vector<TextureSpec> emissionMaps_;  // extension: the emitter shapes' emission maps, in shape order
    EnvironmentSpec environment_;        // extension: the scene file's "environment" block
    int envModeOverride_ = -1;
    bool extensions_ = false, whitted_ = false, hasDielectric_ = false;
    std::vector<VolumeSpec> volumeSpecs_;
    bool volume_ = false, hasVolume_ = false;
    std::vector<size_t> shapeFirstVertex_;  // per entry of the JSON "scene" array (parse() only: setBuffers knows no shapes)
    std::vector<AnimationStep> animation_;
    std::vector<size_t> morphShape_;   // per morph target of the animation file: its shape
    std::vector<float> morphDeltas_;
    bool morphSparse_ = false;  // "sparse_targets": true -- the three arrays below in morphDeltas_' place
    std::vector<uint64_t> morphOffsets_;
    std::vector<uint32_t> morphVertex_;
    std::vector<float> morphSparseDeltas_;
    bool rebuildNormals_ = false;  // "rebuild_normals": true
    unsigned normalFlags_ = 0;     // "weld": "positions" -> GLRTX_NORMALS_WELD_POSITIONS
    VolumeGrid volDensity_, volTemperature_;  // volumeSpecs_[0]'s files (only with enableVolume(true)); only the first volume is rendered (window.cpp:271-286)

    friend class Window;
    friend struct SceneProbe;
    friend struct SceneVolumeProbe;
    friend struct SceneAnimationProbe;
    friend struct SceneMorphProbe;
    friend struct SceneMorphSparseProbe;
    friend struct SceneNormalsProbe;
    friend struct SceneTextureProbe;
    friend struct SceneMapProbe;
    friend struct SceneCutoutProbe;
    friend struct SceneEmissionProbe;
    friend struct SceneEnvironmentProbe;
};

// OBJ triangles the way the reference's loader yields them (trimesh.cpp:113-191): three fresh
// vertices per triangle, file normals normalised, otherwise per-vertex face normals (:38-64).
bool loadObj(const std::string &filename, std::vector<Vertex> &out, std::string &err);

}  // namespace glrt
