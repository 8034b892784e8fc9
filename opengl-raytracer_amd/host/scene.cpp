// scene.cpp -- glrt::Scene::parse and helpers.  Behaviour follows the reference's parser
// (src/core/scene.cpp:31-276) key by key: same required keys (abort on absence), same defaults and
// warnings for optional ones, one material per shape, material id = shape order, light list =
// triangles of shapes with non-zero emission.  Parsers are own code (json.h, loadObj below).
#include "scene.h"

#include <cmath>
#include <cstring>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "glrt_host.h"
#include "glrtx.h"
#include "json.h"
#include "morph_sparse.h"

namespace glrt {

namespace {
std::string dirOf(const std::string &path) {
    const size_t p = path.find_last_of("/\\");
    return p == std::string::npos ? std::string(".") : path.substr(0, p);
}
void vec3(const Json &j, float out[3]) {
    for (int k = 0; k < 3; k++) out[k] = (float)j[(size_t)k].number_value();
}
void fill3(float out[3], float v) { out[0] = out[1] = out[2] = v; }
}  // namespace

Scene::Scene() {
    std::memset(modelM, 0, sizeof modelM);
    std::memset(viewM, 0, sizeof viewM);
    std::memset(projM, 0, sizeof projM);
    for (int i = 0; i < 4; i++) modelM[i * 5] = viewM[i * 5] = projM[i * 5] = 1.0f;
}

Scene::Scene(const std::string &filename) : Scene() { parse(filename); }

void Scene::parse(const std::string &filename) {
    std::ifstream reader(filename.c_str(), std::ios::in);
    if (reader.fail()) GLRT_FatalError("Failed to open file: %s", filename.c_str());
    std::stringstream ss;
    ss << reader.rdbuf();
    std::string err;
    const Json json = Json::parse(ss.str(), err);
    if (!err.empty()) GLRT_Warn("%s", err.c_str());
    const std::string baseDir = dirOf(filename);
    if (const char *e = std::getenv("GLRT_EXTENSIONS")) extensions_ = extensions_ || std::atoi(e) != 0;
    spheres.clear();
    textures_.clear();
    maps_.clear();
    cutouts_.clear();
    emissionMaps_.clear();
    environment_ = EnvironmentSpec{};
    hasDielectric_ = false;
    volumeSpecs_.clear();
    hasVolume_ = false;
    volDensity_ = VolumeGrid{};
    volTemperature_ = VolumeGrid{};

    // film (scene.cpp:57-60)
    width = json["film"]["width"].int_value();
    height = json["film"]["height"].int_value();
    GLRT_Info("window: %d x %d", width, height);

    if (extensions_ && !json["environment"].is_null()) {  // EXTENSION (scene.h: EnvironmentSpec); off, the key is one the parser does not know
        const Json &ev = json["environment"];
        if (!ev.is_object()) GLRT_FatalError("\"environment\" is not an object");
        if (volume_) GLRT_FatalError("\"environment\" and --enable-volume do not combine: the volume branch has its own escape path");
        EnvironmentSpec &spec = environment_;
        if (!ev["file"].is_string() || ev["file"].string_value().empty()) GLRT_FatalError("\"environment\" has no \"file\" string");
        spec.file = baseDir + "/" + ev["file"].string_value();
        const auto word = [&](const char *key, const char *a, const char *b, bool first_default) {
            if (ev[key].is_null()) return first_default;
            const std::string v = ev[key].is_string() ? ev[key].string_value() : std::string();
            if (v != a && v != b) GLRT_FatalError("environment \"%s\" is not \"%s\" or \"%s\"", key, a, b);
            return v == a;
        };
        spec.latlong = word("layout", "latlong", "octahedral", true);
        spec.mode = word("mode", "escape", "sampled", true) ? GLRTX_ENV_ESCAPE : GLRTX_ENV_SAMPLED;
        if (envModeOverride_ >= 0) spec.mode = envModeOverride_;
        spec.filter = word("filter", "bilinear", "nearest", true) ? GLRTX_TEX_BILINEAR : GLRTX_TEX_NEAREST;
        bool srgb = true;
        if (!ev["srgb"].is_null()) {
            if (!ev["srgb"].is_bool()) GLRT_FatalError("environment \"srgb\" is not true or false");
            srgb = ev["srgb"].bool_value();
        }
        if (!ev["scale"].is_null()) {
            if (ev["scale"].is_number()) fill3(spec.scale, (float)ev["scale"].number_value());
            else if (ev["scale"].is_array() && ev["scale"].array_items().size() == 3) vec3(ev["scale"], spec.scale);
            else GLRT_FatalError("environment \"scale\" is not a number or [r, g, b]");
        }
        const auto number = [&](const char *key, float def) {
            if (ev[key].is_null()) return def;
            if (!ev[key].is_number()) GLRT_FatalError("environment \"%s\" is not a number", key);
            return (float)ev[key].number_value();
        };
        spec.rotateY = number("rotate_y", 0.0f);
        spec.lightPick = number("light_pick", 0.5f);
        const int size = (int)number("size", 512.0f);
        TextureImage img;
        std::string terr;
        if (!readTextureFile(spec.file, img, terr)) GLRT_FatalError("environment \"file\": %s", terr.c_str());
        if (spec.latlong) {
            if (size < 2 || size > GLRTX_TEX_MAX_DIM) GLRT_FatalError("environment \"size\" %d lies outside 2 .. %d", size, GLRTX_TEX_MAX_DIM);
            // the picture as float RGB rows from the TOP down (row 0 of the image is the bottom row); a PPM's bytes through the format's own decode
            const size_t n = (size_t)img.width * (size_t)img.height;
            std::vector<float> rgb(3 * n);
            const float *table = glrt_srgb_table();
            for (int y = 0; y < img.height; y++)
                for (int x = 0; x < img.width; x++) {
                    const size_t src = (size_t)(img.height - 1 - y) * img.width + x, dst = (size_t)y * img.width + x;
                    for (int c = 0; c < 3; c++) {
                        if (img.isFloat) std::memcpy(&rgb[3 * dst + c], &img.texels[16 * src + 4 * c], 4);
                        else { const unsigned b = img.texels[4 * src + c]; rgb[3 * dst + c] = srgb ? table[b] : (float)b / 255.0f; }
                    }
                }
            spec.size = size;
            spec.format = GLRTX_TEX_RGBA32F;
            spec.texels.resize((size_t)size * size * 16);
            if (glrt_env_from_latlong(rgb.data(), img.width, img.height, size, reinterpret_cast<float *>(spec.texels.data())) != GLRT_HOST_OK)
                GLRT_FatalError("environment: resampling %s failed", spec.file.c_str());
        } else {
            if (img.width != img.height || img.width < 2) GLRT_FatalError("environment \"file\": an octahedral map is square, 2 texels a side at least (%d x %d)", img.width, img.height);
            spec.size = img.width;
            spec.format = img.isFloat ? GLRTX_TEX_RGBA32F : srgb ? GLRTX_TEX_RGBA8_SRGB : GLRTX_TEX_RGBA8_UNORM;
            spec.texels = std::move(img.texels);
        }
        spec.present = true;
        GLRT_Info("environment: %s, %s, %d x %d octahedral, %s mode (not part of the reference)", spec.file.c_str(), spec.latlong ? "lat-long" : "octahedral",
                  spec.size, spec.size, spec.mode == GLRTX_ENV_SAMPLED ? "sampled" : "escape");
    }

    // camera (scene.cpp:62-114)
    const std::string type = json["camera"]["type"].string_value();
    GLRT_Info("Camera type: %s", type.c_str());
    if (type == "perspective") readPerspective(json["camera"], viewM, projM, apertureRadius, focalLength);

    // shapes (scene.cpp:116-250)
    vertices.clear(); triangles.clear(); lights.clear(); materials.clear(); nodes.clear();
    shapeFirstVertex_.clear(); animation_.clear(); morphShape_.clear(); morphDeltas_.clear();
    morphSparse_ = false; morphOffsets_.clear(); morphVertex_.clear(); morphSparseDeltas_.clear();
    const auto &shapes = json["scene"].array_items();
    for (size_t i = 0; i < shapes.size(); i++) {
        const Json &sh = shapes[i];
        shapeFirstVertex_.push_back(vertices.size());
        const std::string material = sh["material"].string_value();
        Material m;
        std::memset(&m, 0, sizeof m);
        if (material == "diffuse") {
            fill3(m.type, (float)MaterialType::Diffuse);
            if (sh["reflectance"].is_null()) { GLRT_Warn("diffuse node does not have \"reflectance\" key!"); fill3(m.param0, 0.5f); }
            else vec3(sh["reflectance"], m.param0);
            if (extensions_ && !sh["texture"].is_null()) {  // EXTENSION (scene.h: TextureSpec); off, the key is one the parser does not know
                const Json &tx = sh["texture"];
                if (!tx.is_object()) GLRT_FatalError("shape %zu: \"texture\" is not an object", i);
                TextureSpec spec;
                spec.material = materials.size();
                if (!tx["file"].is_string() || tx["file"].string_value().empty()) GLRT_FatalError("shape %zu: \"texture\" has no \"file\" string", i);
                spec.file = baseDir + "/" + tx["file"].string_value();
                spec.filter = GLRTX_TEX_BILINEAR;
                if (!tx["filter"].is_null()) {
                    const std::string v = tx["filter"].is_string() ? tx["filter"].string_value() : std::string();
                    if (v == "bilinear") spec.filter = GLRTX_TEX_BILINEAR;
                    else if (v == "nearest") spec.filter = GLRTX_TEX_NEAREST;
                    else GLRT_FatalError("shape %zu: texture \"filter\" is not \"bilinear\" or \"nearest\"", i);
                }
                spec.wrap = GLRTX_TEX_REPEAT;
                if (!tx["wrap"].is_null()) {
                    const std::string v = tx["wrap"].is_string() ? tx["wrap"].string_value() : std::string();
                    if (v == "repeat") spec.wrap = GLRTX_TEX_REPEAT;
                    else if (v == "clamp") spec.wrap = GLRTX_TEX_CLAMP;
                    else GLRT_FatalError("shape %zu: texture \"wrap\" is not \"repeat\" or \"clamp\"", i);
                }
                bool srgb = true;
                if (!tx["srgb"].is_null()) {
                    if (!tx["srgb"].is_bool()) GLRT_FatalError("shape %zu: texture \"srgb\" is not true or false", i);
                    srgb = tx["srgb"].bool_value();
                }
                std::string terr;
                if (!readTextureFile(spec.file, spec.image, terr)) GLRT_FatalError("shape %zu: texture \"file\": %s", i, terr.c_str());
                spec.format = spec.image.isFloat ? GLRTX_TEX_RGBA32F : srgb ? GLRTX_TEX_RGBA8_SRGB : GLRTX_TEX_RGBA8_UNORM;
                GLRT_Info("texture: %s, %d x %d, %s", spec.file.c_str(), spec.image.width, spec.image.height,
                          spec.image.isFloat ? "float" : srgb ? "8-bit sRGB" : "8-bit linear");
                textures_.push_back(std::move(spec));
            }
        } else if (material == "conductor") {
            fill3(m.type, (float)MaterialType::Conductor);
            if (sh["kappa"].is_null()) { GLRT_Warn("conductor node does not have \"kappa\" key!"); fill3(m.param0, 1.0f); }
            else vec3(sh["kappa"], m.param0);
            if (sh["eta"].is_null()) { GLRT_Warn("conductor node does not have \"eta\" key!"); fill3(m.param1, 1.0f); }
            else vec3(sh["eta"], m.param1);
            if (sh["alpha"].is_null()) { GLRT_Warn("conductor node does not have \"alpha\" key!"); fill3(m.param2, 0.0f); }
            else fill3(m.param2, (float)sh["alpha"].number_value());
        } else if (material == "emitter") {
            fill3(m.type, (float)MaterialType::Emitter);
            if (sh["emission"].is_null()) GLRT_Warn("emitter node does not have \"emission\" key!");
            else vec3(sh["emission"], m.emission);
            if (extensions_ && !sh["emission_map"].is_null()) {  // EXTENSION (scene.h: emissionMapSpecs); off, the key is one the parser does not know
                const Json &tx = sh["emission_map"];
                if (!tx.is_object()) GLRT_FatalError("shape %zu: \"emission_map\" is not an object", i);
                TextureSpec spec;
                spec.material = materials.size();
                if (!tx["file"].is_string() || tx["file"].string_value().empty()) GLRT_FatalError("shape %zu: \"emission_map\" has no \"file\" string", i);
                spec.file = baseDir + "/" + tx["file"].string_value();
                spec.filter = GLRTX_TEX_BILINEAR;
                if (!tx["filter"].is_null()) {
                    const std::string v = tx["filter"].is_string() ? tx["filter"].string_value() : std::string();
                    if (v == "bilinear") spec.filter = GLRTX_TEX_BILINEAR;
                    else if (v == "nearest") spec.filter = GLRTX_TEX_NEAREST;
                    else GLRT_FatalError("shape %zu: emission_map \"filter\" is not \"bilinear\" or \"nearest\"", i);
                }
                spec.wrap = GLRTX_TEX_REPEAT;
                if (!tx["wrap"].is_null()) {
                    const std::string v = tx["wrap"].is_string() ? tx["wrap"].string_value() : std::string();
                    if (v == "repeat") spec.wrap = GLRTX_TEX_REPEAT;
                    else if (v == "clamp") spec.wrap = GLRTX_TEX_CLAMP;
                    else GLRT_FatalError("shape %zu: emission_map \"wrap\" is not \"repeat\" or \"clamp\"", i);
                }
                bool srgb = true;
                if (!tx["srgb"].is_null()) {
                    if (!tx["srgb"].is_bool()) GLRT_FatalError("shape %zu: emission_map \"srgb\" is not true or false", i);
                    srgb = tx["srgb"].bool_value();
                }
                std::string terr;
                if (!readTextureFile(spec.file, spec.image, terr)) GLRT_FatalError("shape %zu: emission_map \"file\": %s", i, terr.c_str());
                spec.format = spec.image.isFloat ? GLRTX_TEX_RGBA32F : srgb ? GLRTX_TEX_RGBA8_SRGB : GLRTX_TEX_RGBA8_UNORM;
                GLRT_Info("emission map: %s, %d x %d, %s", spec.file.c_str(), spec.image.width, spec.image.height,
                          spec.image.isFloat ? "float" : srgb ? "8-bit sRGB" : "8-bit linear");
                emissionMaps_.push_back(std::move(spec));
            }
        } else if (material == "media") {
            // The reference uploads two 3D textures here, but its shader's volume branch is compiled
            // out (raytrace.frag:4, :424-487): the material only marks the surface as pass-through -- unless enableVolume(true).
            fill3(m.type, (float)MaterialType::Media);
            const Json &vol = sh["volume"];
            if (vol.is_object()) {
                VolumeSpec spec;
                spec.density = baseDir + "/" + vol["density"].string_value();
                spec.temperature = baseDir + "/" + vol["temperature"].string_value();
                fill3(spec.bboxMin, 0.0f);
                fill3(spec.bboxMax, 0.0f);
                if (vol["bboxMin"].is_null()) GLRT_Warn("volume node does not have \"bboxMin\" key!");
                else vec3(vol["bboxMin"], spec.bboxMin);
                if (vol["bboxMax"].is_null()) GLRT_Warn("volume node does not have \"bboxMax\" key!");
                else vec3(vol["bboxMax"], spec.bboxMax);
                volumeSpecs_.push_back(spec);
                if (volume_ && volumeSpecs_.size() == 1) {  // only volumes[0] is ever bound (window.cpp:271-286)
                    std::string verr;
                    if (!readVol(spec.density, volDensity_, verr)) GLRT_FatalError("Failed to load volume: %s", verr.c_str());
                    if (!readVol(spec.temperature, volTemperature_, verr)) GLRT_FatalError("Failed to load volume: %s", verr.c_str());
                    if (volDensity_.nx != volTemperature_.nx || volDensity_.ny != volTemperature_.ny || volDensity_.nz != volTemperature_.nz)
                        GLRT_FatalError("volume: density (%dx%dx%d) and temperature (%dx%dx%d) grids differ in size", volDensity_.nx, volDensity_.ny,
                                        volDensity_.nz, volTemperature_.nx, volTemperature_.ny, volTemperature_.nz);
                    hasVolume_ = true;
                }
            }
        } else if (material == "dielectric" && extensions_) {
            // EXTENSION (no reference counterpart): MTRL_DIELECTRIC = 4 (raytrace.frag:32); param0 = tint, param1.x = index of refraction
            fill3(m.type, 4.0f);
            if (sh["tint"].is_null()) fill3(m.param0, 1.0f);
            else vec3(sh["tint"], m.param0);
            fill3(m.param1, 0.0f);
            m.param1[0] = sh["ior"].is_null() ? 1.5f : (float)sh["ior"].number_value();
            hasDielectric_ = true;
        } else {
            GLRT_FatalError("Unsupported material: %s", material.c_str());
        }
        if (extensions_) {  // EXTENSION (scene.h: MapSpec); off, the keys are ones the parser does not know
            for (const char *key : {"normal_map", "roughness_map"}) {
                const Json &mp = sh[key];
                if (mp.is_null()) continue;
                const bool rough = key[0] == 'r';
                if (!mp.is_object()) GLRT_FatalError("shape %zu: \"%s\" is not an object", i, key);
                if (rough ? material != "conductor" : (material != "diffuse" && material != "conductor"))
                    GLRT_FatalError("shape %zu: \"%s\" on a %s shape (%s)", i, key, material.c_str(), rough ? "a conductor takes one" : "a diffuse or conductor shape takes one");
                MapSpec spec;
                spec.material = materials.size();
                spec.roughness = rough;
                if (!mp["file"].is_string() || mp["file"].string_value().empty()) GLRT_FatalError("shape %zu: \"%s\" has no \"file\" string", i, key);
                spec.file = baseDir + "/" + mp["file"].string_value();
                spec.filter = GLRTX_TEX_BILINEAR;
                if (!mp["filter"].is_null()) {
                    const std::string v = mp["filter"].is_string() ? mp["filter"].string_value() : std::string();
                    if (v == "bilinear") spec.filter = GLRTX_TEX_BILINEAR;
                    else if (v == "nearest") spec.filter = GLRTX_TEX_NEAREST;
                    else GLRT_FatalError("shape %zu: %s \"filter\" is not \"bilinear\" or \"nearest\"", i, key);
                }
                spec.wrap = GLRTX_TEX_REPEAT;
                if (!mp["wrap"].is_null()) {
                    const std::string v = mp["wrap"].is_string() ? mp["wrap"].string_value() : std::string();
                    if (v == "repeat") spec.wrap = GLRTX_TEX_REPEAT;
                    else if (v == "clamp") spec.wrap = GLRTX_TEX_CLAMP;
                    else GLRT_FatalError("shape %zu: %s \"wrap\" is not \"repeat\" or \"clamp\"", i, key);
                }
                if (!mp["srgb"].is_null() && !(mp["srgb"].is_bool() && !mp["srgb"].bool_value()))
                    GLRT_FatalError("shape %zu: %s \"srgb\": a map holds vectors, not colours (an sRGB map is refused)", i, key);
                spec.scale = 1.0f;
                if (!mp["scale"].is_null()) {
                    if (rough) GLRT_FatalError("shape %zu: roughness_map has no \"scale\"", i);
                    spec.scale = mp["scale"].is_number() ? (float)mp["scale"].number_value() : NAN;
                    if (!std::isfinite(spec.scale)) GLRT_FatalError("shape %zu: normal_map \"scale\" is not a finite number", i);
                }
                std::string terr;
                if (!readTextureFile(spec.file, spec.image, terr)) GLRT_FatalError("shape %zu: %s \"file\": %s", i, key, terr.c_str());
                spec.format = spec.image.isFloat ? GLRTX_TEX_RGBA32F : GLRTX_TEX_RGBA8_UNORM;
                GLRT_Info("%s: %s, %d x %d, %s", key, spec.file.c_str(), spec.image.width, spec.image.height, spec.image.isFloat ? "float" : "8-bit linear");
                maps_.push_back(std::move(spec));
            }
        }
        if (extensions_ && !sh["cutout"].is_null()) {  // EXTENSION (scene.h: CutoutSpec); off, the key is one the parser does not know
            const Json &ct = sh["cutout"];
            if (!ct.is_object()) GLRT_FatalError("shape %zu: \"cutout\" is not an object", i);
            if (material != "diffuse" && material != "conductor")
                GLRT_FatalError("shape %zu: \"cutout\" on a %s shape (a diffuse or conductor shape takes one)", i, material.c_str());
            CutoutSpec spec;
            spec.material = materials.size();
            if (!ct["file"].is_string() || ct["file"].string_value().empty()) GLRT_FatalError("shape %zu: \"cutout\" has no \"file\" string", i);
            spec.file = baseDir + "/" + ct["file"].string_value();
            spec.filter = GLRTX_TEX_BILINEAR;
            if (!ct["filter"].is_null()) {
                const std::string v = ct["filter"].is_string() ? ct["filter"].string_value() : std::string();
                if (v == "bilinear") spec.filter = GLRTX_TEX_BILINEAR;
                else if (v == "nearest") spec.filter = GLRTX_TEX_NEAREST;
                else GLRT_FatalError("shape %zu: cutout \"filter\" is not \"bilinear\" or \"nearest\"", i);
            }
            spec.wrap = GLRTX_TEX_REPEAT;
            if (!ct["wrap"].is_null()) {
                const std::string v = ct["wrap"].is_string() ? ct["wrap"].string_value() : std::string();
                if (v == "repeat") spec.wrap = GLRTX_TEX_REPEAT;
                else if (v == "clamp") spec.wrap = GLRTX_TEX_CLAMP;
                else GLRT_FatalError("shape %zu: cutout \"wrap\" is not \"repeat\" or \"clamp\"", i);
            }
            if (!ct["srgb"].is_null() && !(ct["srgb"].is_bool() && !ct["srgb"].bool_value()))
                GLRT_FatalError("shape %zu: cutout \"srgb\": a mask holds coverage, not colour (an sRGB mask is refused)", i);
            spec.channel = 0;
            if (!ct["channel"].is_null()) {
                const std::string v = ct["channel"].is_string() ? ct["channel"].string_value() : std::string();
                if (v == "r") spec.channel = 0;
                else if (v == "g") spec.channel = 1;
                else if (v == "b") spec.channel = 2;
                else GLRT_FatalError("shape %zu: cutout \"channel\" is not \"r\", \"g\" or \"b\" (the image readers are three-channel)", i);
            }
            spec.cutoff = 0.5f;
            if (!ct["cutoff"].is_null()) {
                const double v = ct["cutoff"].is_number() ? ct["cutoff"].number_value() : (double)NAN;
                if (!(std::fabs(v) <= 3.4028234663852886e38)) GLRT_FatalError("shape %zu: cutout \"cutoff\" is not a finite number", i);  // (a float's range; NaN fails too)
                spec.cutoff = (float)v;
            }
            std::string terr;
            if (!readTextureFile(spec.file, spec.image, terr)) GLRT_FatalError("shape %zu: cutout \"file\": %s", i, terr.c_str());
            spec.format = spec.image.isFloat ? GLRTX_TEX_RGBA32F : GLRTX_TEX_RGBA8_UNORM;
            GLRT_Info("cutout: %s, %d x %d, %s, channel %d, cutoff %g", spec.file.c_str(), spec.image.width, spec.image.height, spec.image.isFloat ? "float" : "8-bit linear",
                      spec.channel, (double)spec.cutoff);
            cutouts_.push_back(std::move(spec));
        }
        materials.push_back(m);

        if (sh["type"].string_value() == "obj") {
            const std::string file = baseDir + "/" + sh["filename"].string_value();
            std::vector<Vertex> mesh;
            std::string oerr;
            if (!loadObj(file, mesh, oerr)) GLRT_FatalError("Failed to load *.obj file: %s (%s)", file.c_str(), oerr.c_str());
            const size_t base = vertices.size();
            vertices.insert(vertices.end(), mesh.begin(), mesh.end());
            for (size_t t = 0; t + 2 < mesh.size(); t += 3) {
                Triangle tri;
                tri.indices[0] = (float)(base + t);
                tri.indices[1] = (float)(base + t + 1);
                tri.indices[2] = (float)(base + t + 2);
                tri.indices[3] = (float)(materials.size() - 1);
                triangles.push_back(tri);
            }
        } else if (sh["type"].string_value() == "sphere" && extensions_) {  // EXTENSION: analytic sphere
            float ctr[3] = {0.f, 0.f, 0.f};
            if (!sh["center"].is_null()) vec3(sh["center"], ctr);
            const float radius = sh["radius"].is_null() ? 1.0f : (float)sh["radius"].number_value();
            if (!(radius > 0.0f)) GLRT_FatalError("sphere radius must be positive");
            spheres.insert(spheres.end(), {ctr[0], ctr[1], ctr[2], radius, (float)(materials.size() - 1)});
        }
    }
    finalize();
    GLRT_Info("Scene setup OK!");
    GLRT_Info("#vertex: %d", (int)vertices.size());
    GLRT_Info("#triangle: %d", (int)triangles.size());
    GLRT_Info("#BVH node: %d", (int)nodes.size());
}

void Scene::readPerspective(const Json &cam, float view[16], float proj[16], float &aperture, float &focal) const {
    aperture = (float)cam["apertureRadius"].number_value();  // absent -> 0
    focal = (float)cam["focalLength"].number_value();        // absent -> 0 (scene.cpp:71-74)
    if (cam["lookAt"].is_null()) GLRT_FatalError("perspective camera node does not have \"lookAt\" key!");
    float origin[3], target[3], up[3];
    vec3(cam["lookAt"]["origin"], origin);
    vec3(cam["lookAt"]["target"], target);
    vec3(cam["lookAt"]["up"], up);
    glrt_look_at(origin, target, up, view);
    if (cam["fov"].is_null()) GLRT_FatalError("perspective camera node does not have \"fov\" key!");
    if (cam["nearClip"].is_null()) GLRT_FatalError("perspective camera node does not have \"nearClip\" key!");
    if (cam["farClip"].is_null()) GLRT_FatalError("perspective camera node does not have \"farClip\" key!");
    glrt_perspective((float)cam["fov"].number_value(), (float)width / (float)height,
                     (float)cam["nearClip"].number_value(), (float)cam["farClip"].number_value(), proj);
}

void Scene::parseAnimation(const std::string &filename) {
    std::ifstream reader(filename.c_str(), std::ios::in);
    if (reader.fail()) GLRT_FatalError("Failed to open file: %s", filename.c_str());
    std::stringstream ss;
    ss << reader.rdbuf();
    std::string err;
    const Json json = Json::parse(ss.str(), err);
    if (!err.empty()) GLRT_FatalError("animation: %s", err.c_str());
    if (!json["steps"].is_array()) GLRT_FatalError("animation: no \"steps\" array");
    const size_t n_shapes = shapeFirstVertex_.size();
    animation_.clear(); morphShape_.clear(); morphDeltas_.clear();
    morphSparse_ = false; morphOffsets_.clear(); morphVertex_.clear(); morphSparseDeltas_.clear();
    if (!json["sparse_targets"].is_null() && !json["sparse_targets"].is_bool()) GLRT_FatalError("animation: \"sparse_targets\" is not true or false");
    morphSparse_ = json["sparse_targets"].bool_value();
    if (!json["rebuild_normals"].is_null() && !json["rebuild_normals"].is_bool()) GLRT_FatalError("animation: \"rebuild_normals\" is not true or false");
    rebuildNormals_ = json["rebuild_normals"].bool_value();
    normalFlags_ = 0;
    if (!json["weld"].is_null()) {
        const std::string weld = json["weld"].string_value();
        if (!json["weld"].is_string() || (weld != "positions" && weld != "normals"))
            GLRT_FatalError("animation: \"weld\" is not \"positions\" or \"normals\"");
        if (weld == "positions") normalFlags_ = GLRT_NORMALS_WELD_POSITIONS;
    }
    auto index_of = [](const Json &x, size_t n) { const double v = x.number_value(); return x.is_number() && v >= 0.0 && v < (double)n && v == std::floor(v); };
    if (!json["targets"].is_null()) {  // morph targets: one OBJ a target, the deltas of its shape's vertices
        if (!json["targets"].is_array()) GLRT_FatalError("animation: \"targets\" is not an array");
        const auto &targets = json["targets"].array_items();
        if (morphSparse_ && targets.size() > GLRT_MAX_SPARSE_MORPH_TARGETS)
            GLRT_FatalError("animation: %zu sparse morph targets (at most %d)", targets.size(), GLRT_MAX_SPARSE_MORPH_TARGETS);
        if (!morphSparse_ && targets.size() > 64) GLRT_FatalError("animation: %zu morph targets (at most 64)", targets.size());
        const size_t slash = filename.find_last_of("/\\");
        const std::string dir = slash == std::string::npos ? "." : filename.substr(0, slash);
        if (morphSparse_) morphOffsets_.assign(1, 0);  // (the dense targets x vertices x 6 array is never allocated)
        else morphDeltas_.assign(targets.size() * vertices.size() * 6, 0.0f);
        for (size_t t = 0; t < targets.size(); t++) {
            if (!index_of(targets[t]["shape"], n_shapes))
                GLRT_FatalError("animation target %zu: shape index %g is out of range (the scene has %zu shapes)", t, targets[t]["shape"].number_value(), n_shapes);
            const size_t shape = (size_t)targets[t]["shape"].number_value();
            const std::string file = dir + "/" + targets[t]["file"].string_value();
            std::vector<Vertex> mesh;
            std::string oerr;
            if (!loadObj(file, mesh, oerr)) GLRT_FatalError("animation target %zu: failed to load *.obj file: %s (%s)", t, file.c_str(), oerr.c_str());
            const size_t first = shapeFirstVertex(shape), count = shapeFirstVertex(shape + 1) - first;
            if (mesh.size() != count)
                GLRT_FatalError("animation target %zu: %s has %zu vertices, shape %zu has %zu", t, file.c_str(), mesh.size(), shape, count);
            if (morphSparse_) {  // the index directly: a vertex of the shape gets an entry iff its delta passes glrt_morph_sparsify's rule
                for (size_t v = 0; v < count; v++) {
                    float d[6];
                    for (int k = 0; k < 3; k++) {
                        d[k] = mesh[v].pos[k] - vertices[first + v].pos[k];
                        d[3 + k] = mesh[v].normal[k] - vertices[first + v].normal[k];
                    }
                    if (!glrt_detail::morph_entry_kept(d)) continue;
                    morphVertex_.push_back((uint32_t)(first + v));
                    morphSparseDeltas_.insert(morphSparseDeltas_.end(), d, d + 6);
                }
                morphOffsets_.push_back((uint64_t)morphVertex_.size());
                morphShape_.push_back(shape);
                continue;
            }
            float *d = morphDeltas_.data() + (t * vertices.size() + first) * 6;
            for (size_t v = 0; v < count; v++)
                for (int k = 0; k < 3; k++) {
                    d[6 * v + k] = mesh[v].pos[k] - vertices[first + v].pos[k];
                    d[6 * v + 3 + k] = mesh[v].normal[k] - vertices[first + v].normal[k];
                }
            morphShape_.push_back(shape);
        }
    }
    const size_t n_targets = morphShape_.size();
    const auto &steps = json["steps"].array_items();
    for (size_t s = 0; s < steps.size(); s++) {
        AnimationStep st;
        st.matrices.assign(12 * n_shapes, 0.0f);
        for (size_t b = 0; b < n_shapes; b++) st.matrices[12 * b] = st.matrices[12 * b + 5] = st.matrices[12 * b + 10] = 1.0f;
        for (const Json &entry : steps[s]["matrices"].array_items()) {
            const auto &v = entry.array_items();
            bool numbers = true;
            for (const Json &x : v) numbers = numbers && x.is_number();
            if (v.size() != 13 || !numbers)
                GLRT_FatalError("animation step %zu: a matrix entry is a shape index and 12 numbers, this one has %zu", s, v.empty() ? (size_t)0 : v.size() - 1);
            const double shape = v[0].number_value();
            if (!(shape >= 0.0 && shape < (double)n_shapes) || shape != std::floor(shape))
                GLRT_FatalError("animation step %zu: shape index %g is out of range (the scene has %zu shapes)", s, shape, n_shapes);
            for (size_t k = 0; k < 12; k++) st.matrices[12 * (size_t)shape + k] = (float)v[k + 1].number_value();
        }
        st.weights.assign(n_targets, 0.0f);
        for (const Json &entry : steps[s]["weights"].array_items()) {
            const auto &v = entry.array_items();
            if (v.size() != 2 || !v[1].is_number()) GLRT_FatalError("animation step %zu: a weight entry is a target index and a number", s);
            if (!index_of(v[0], n_targets))
                GLRT_FatalError("animation step %zu: target index %g is out of range (the file has %zu targets)", s, v[0].number_value(), n_targets);
            st.weights[(size_t)v[0].number_value()] = (float)v[1].number_value();
        }
        const Json &cam = steps[s]["camera"];
        if (!cam.is_null()) {
            if (cam["type"].string_value() != "perspective") GLRT_FatalError("animation step %zu: camera type \"%s\" (perspective)", s, cam["type"].string_value().c_str());
            st.hasCamera = true;
            readPerspective(cam, st.viewM, st.projM, st.apertureRadius, st.focalLength);
        }
        animation_.push_back(std::move(st));
    }
    GLRT_Info("Animation: %zu steps, %zu shapes", animation_.size(), n_shapes);
    if (n_targets && morphSparse_) GLRT_Info("Animation: %zu sparse morph targets, %zu entries", n_targets, morphVertex_.size());
    else if (n_targets) GLRT_Info("Animation: %zu morph targets", n_targets);
    if (rebuildNormals_) GLRT_Info("Animation: normals rebuilt from the moved faces, welded by %s", normalFlags_ ? "position" : "position and normal");
}

void Scene::setBuffers(int w, int h, const float view[16], const float proj[16], float aperture, float focal,
                       std::vector<Vertex> v, std::vector<Triangle> t, std::vector<Material> m, std::vector<BVHNode> n) {
    width = w; height = h; apertureRadius = aperture; focalLength = focal;
    std::memcpy(viewM, view, sizeof viewM);
    std::memcpy(projM, proj, sizeof projM);
    vertices = std::move(v); triangles = std::move(t); materials = std::move(m); nodes = std::move(n);
    shapeFirstVertex_.clear(); animation_.clear(); morphShape_.clear(); morphDeltas_.clear();
    morphSparse_ = false; morphOffsets_.clear(); morphVertex_.clear(); morphSparseDeltas_.clear();
    finalize();
}

void Scene::finalize() {
    lights.clear();
    for (const Triangle &t : triangles) {
        const size_t m = (size_t)t.indices[3];
        if (m < materials.size()) {
            const float *e = materials[m].emission;
            if (std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) != 0.0f) lights.push_back(t);  // scene.cpp:246-248
        }
    }
    if (nodes.empty() && !triangles.empty()) {
        // BVH::construct (scene.cpp:251-253 -> bvh.cpp:59-160).  Builders: "sah" (CPU, default), "sah-gpu" (binned SAH by levels + exact sweep below, built on the
        // GPU through glrtx_build_bvh_sah: the CPU SAH tree's quality in ~1.3 ms per 100 k triangles), "lbvh" (linear BVH
        // built on the GPU through glrtx_build_lbvh: 20 % faster to build, ~3 % more traversal steps), "sah-levels-cpu" / "lbvh-cpu" (the same trees from the host library),
        // "sah-reinsert" ("sah" + glrt_bvh_reinsert: config 5 renders 3 % faster, the build takes seconds), "reference" (the reference host's OWN tree, its builder
        // restated rule for rule -- glrt_host.h: glrt_bvh_build_reference -- and left in its own child order: exact ties and grazing-ray box misses then fall where the
        // reference host's do).  Any of them renders the same image except at those two kinds of pixels.
        std::string kind = bvhBuilder_;
        if (const char *e = std::getenv("GLRT_BVH")) kind = e;
        nodes.resize(glrt_bvh_node_count(triangles.size()));
        const float *v = &vertices[0].pos[0], *t = &triangles[0].indices[0];
        if (kind == "sah" || kind == "sah-reinsert" || kind == "lbvh-cpu" || kind == "sah-levels-cpu" || kind == "reference") {
            const int rc = kind == "sah" || kind == "sah-reinsert" ? glrt_bvh_build_sah(v, vertices.size(), t, triangles.size(), &nodes[0].bboxMin[0], &bvhDepth_)
                         : kind == "reference" ? glrt_bvh_build_reference(v, vertices.size(), t, triangles.size(), &nodes[0].bboxMin[0], &bvhDepth_)
                         : kind == "lbvh-cpu" ? glrt_bvh_build_lbvh(v, vertices.size(), t, triangles.size(), &nodes[0].bboxMin[0], &bvhDepth_)
                                              : glrt_bvh_build_sah_levels(v, vertices.size(), t, triangles.size(), &nodes[0].bboxMin[0], &bvhDepth_);
            if (rc != GLRT_HOST_OK) GLRT_FatalError("BVH construction (%s) failed (%d)", kind.c_str(), rc);
            if (kind == "sah-reinsert") {  // insertion-based optimisation of the finished tree (glrt_host.h: glrt_bvh_reinsert): ~3 % fewer box visits on config 5, seconds of CPU
                double cost[2] = {0.0, 0.0};
                int depth = -1;
                const int moved = glrt_bvh_reinsert(&nodes[0].bboxMin[0], nodes.size(), 8, &depth, cost);
                if (moved == GLRT_HOST_EDEPTH) {  // the optimised tree would not fit the traversal stack: the pass has put the SAH tree back (glrt_host.h)
                    GLRT_Info("BVH: reinsertion would deepen the tree to %d levels (the traversal stack holds 64 entries): keeping the SAH tree", depth);
                    depth = -1;
                } else if (moved < 0) GLRT_FatalError("glrt_bvh_reinsert failed (%d)", moved);
                if (depth >= 0) bvhDepth_ = depth;
                if (moved >= 0) GLRT_Info("BVH: %d subtrees reinserted, summed fork area %.2f -> %.2f root areas (depth %d)", moved, cost[0], cost[1], bvhDepth_);
            }
        } else if (kind == "lbvh" || kind == "sah-gpu") {
            glrtx_ctx *ctx = nullptr;
            if (glrtx_create(&ctx, -1) != GLRTX_OK) GLRT_FatalError("GPU BVH builder: %s", glrtx_last_error(nullptr));
            float ms = 0.0f;
            const int rc = kind == "lbvh" ? glrtx_build_lbvh(ctx, v, vertices.size(), t, triangles.size(), &nodes[0].bboxMin[0], &bvhDepth_, &ms)
                                          : glrtx_build_bvh_sah(ctx, v, vertices.size(), t, triangles.size(), &nodes[0].bboxMin[0], &bvhDepth_, &ms);
            if (rc != GLRTX_OK) GLRT_FatalError("GPU BVH builder (%s): %s", kind.c_str(), glrtx_last_error(ctx));
            GLRT_Info("%s over %zu triangles built on the GPU in %.3f ms (depth %d)", kind == "lbvh" ? "LBVH" : "SAH tree", triangles.size(), ms, bvhDepth_);
            glrtx_destroy(ctx);
        } else {
            GLRT_FatalError("unknown BVH builder '%s' (sah | sah-reinsert | sah-gpu | lbvh | sah-levels-cpu | lbvh-cpu | reference)", kind.c_str());
        }
        // the light side first: at a fork where only one child holds emitting triangles that child is visited first (glrt_host.h: glrt_bvh_lights_first)
        const char *lf = std::getenv("GLRT_BVH_LIGHTS_FIRST");
        if (kind == "reference") {
            GLRT_Info("BVH: the reference host's own tree (bvh.cpp:72-160 restated), left in its own child order (depth %d)", bvhDepth_);
        } else if (!(lf && lf[0] == '0' && lf[1] == 0) && !materials.empty()) {
            const int sw = glrt_bvh_lights_first(&nodes[0].bboxMin[0], nodes.size(), t, triangles.size(), &materials[0].type[0], materials.size());
            if (sw < 0) GLRT_FatalError("glrt_bvh_lights_first failed (%d)", sw);
            if (sw > 0) GLRT_Info("BVH: the light side first at %d forks", sw);
        }
    }
}

// ------------------------------------------------------------------------------------------------ OBJ
bool loadObj(const std::string &filename, std::vector<Vertex> &out, std::string &err) {
    std::ifstream in(filename.c_str());
    if (in.fail()) { err = "cannot open"; return false; }
    std::vector<float> P, N, T;
    struct Corner { int v, t, n; };
    std::vector<Corner> corners;  // 3 per triangle
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string tag;
        if (!(ls >> tag) || tag[0] == '#') continue;
        if (tag == "v") { float x, y, z; ls >> x >> y >> z; P.insert(P.end(), {x, y, z}); }
        else if (tag == "vn") { float x, y, z; ls >> x >> y >> z; N.insert(N.end(), {x, y, z}); }
        else if (tag == "vt") { float u = 0, v = 0; ls >> u >> v; T.insert(T.end(), {u, v}); }
        else if (tag == "f") {
            std::vector<Corner> poly;
            std::string tok;
            while (ls >> tok) {
                Corner c{-1, -1, -1};
                int *slot[3] = {&c.v, &c.t, &c.n};
                size_t s = 0;
                for (int k = 0; k < 3 && s <= tok.size(); k++) {
                    const size_t e = tok.find('/', s);
                    const std::string part = tok.substr(s, e == std::string::npos ? std::string::npos : e - s);
                    if (!part.empty()) {
                        const int idx = std::atoi(part.c_str());
                        const int count = (int)((k == 0 ? P.size() / 3 : k == 1 ? T.size() / 2 : N.size() / 3));
                        *slot[k] = idx > 0 ? idx - 1 : count + idx;  // negative = relative to the end
                    }
                    if (e == std::string::npos) break;
                    s = e + 1;
                }
                poly.push_back(c);
            }
            for (size_t k = 1; k + 1 < poly.size(); k++) {  // fan triangulation
                corners.push_back(poly[0]); corners.push_back(poly[k]); corners.push_back(poly[k + 1]);
            }
        }
    }
    bool hasNorm = !corners.empty(), hasUV = !corners.empty();
    out.clear();
    out.reserve(corners.size());
    for (const Corner &c : corners) {
        Vertex v;
        std::memset(&v, 0, sizeof v);
        if (c.v < 0 || (size_t)c.v * 3 + 2 >= P.size()) { err = "vertex index out of range"; return false; }
        std::memcpy(v.pos, &P[(size_t)c.v * 3], 12);
        if (c.n >= 0 && (size_t)c.n * 3 + 2 < N.size()) {
            const float *n = &N[(size_t)c.n * 3];
            const float l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int k = 0; k < 3; k++) v.normal[k] = n[k] / l;  // normalised on load (trimesh.cpp:162)
        } else {
            hasNorm = false;
        }
        if (c.t >= 0 && (size_t)c.t * 2 + 1 < T.size()) { v.uv[0] = T[(size_t)c.t * 2]; v.uv[1] = T[(size_t)c.t * 2 + 1]; }
        else hasUV = false;
        out.push_back(v);
    }
    if (!hasNorm) {  // face normals accumulated per vertex (trimesh.cpp:38-64); vertices are not shared
        for (size_t t = 0; t + 2 < out.size(); t += 3) {
            const float *a = out[t].pos, *b = out[t + 1].pos, *c = out[t + 2].pos;
            const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const float l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int k = 0; k < 3; k++) n[k] = l != 0.0f ? n[k] / l : 0.0f;
            for (int q = 0; q < 3; q++) std::memcpy(out[t + q].normal, n, 12);
        }
    }
    if (hasUV) {
        // Tangent frame from the texture coordinates (trimesh.cpp:67-110), carried in texels 3 and 4 of the vertex record.  The path tracer never reads them
        // (raytrace.frag:316-321 fetches texels 0 and 1 only); they are filled so that the vertex buffer a Scene hands over is the reference's record for record.
        // Per face: the reference's (-dP1 dv2 + dP2 dv1) / det and (-dP2 du1 + dP1 du2) / det -- the NEGATED derivatives of the position along u and v, as written there --, each normalised; a vertex sums its faces' (here: its one face's -- vertices are not shared) and
        // normalises the sums where both are non-zero.  A face whose texture coordinates are collinear (zero determinant) contributes nothing.
        for (size_t t = 0; t + 2 < out.size(); t += 3) {
            const Vertex &a = out[t], &b = out[t + 1], &c = out[t + 2];
            const float p1[3] = {b.pos[0] - a.pos[0], b.pos[1] - a.pos[1], b.pos[2] - a.pos[2]}, p2[3] = {c.pos[0] - a.pos[0], c.pos[1] - a.pos[1], c.pos[2] - a.pos[2]};
            const float du1 = b.uv[0] - a.uv[0], dv1 = b.uv[1] - a.uv[1], du2 = c.uv[0] - a.uv[0], dv2 = c.uv[1] - a.uv[1];
            const float det = du1 * dv2 - dv1 * du2;
            if (det == 0.0f) continue;
            float tg[3], bn[3];
            for (int k = 0; k < 3; k++) {
                tg[k] = (-p1[k] * dv2 + p2[k] * dv1) / det;
                bn[k] = (-p2[k] * du1 + p1[k] * du2) / det;
            }
            const float lt = std::sqrt(tg[0] * tg[0] + tg[1] * tg[1] + tg[2] * tg[2]), lb = std::sqrt(bn[0] * bn[0] + bn[1] * bn[1] + bn[2] * bn[2]);
            for (int q = 0; q < 3; q++)
                for (int k = 0; k < 3; k++) { out[t + q].tangent[k] += tg[k] / lt; out[t + q].binormal[k] += bn[k] / lb; }
        }
        for (Vertex &v : out) {
            const float lt = std::sqrt(v.tangent[0] * v.tangent[0] + v.tangent[1] * v.tangent[1] + v.tangent[2] * v.tangent[2]);
            const float lb = std::sqrt(v.binormal[0] * v.binormal[0] + v.binormal[1] * v.binormal[1] + v.binormal[2] * v.binormal[2]);
            if (lt > 0.0f && lb > 0.0f)
                for (int k = 0; k < 3; k++) { v.tangent[k] /= lt; v.binormal[k] /= lb; }
        }
    }
    return true;
}

}  // namespace glrt

// ---------------------------------------------------------------------------------------------- test hook
// Host-only probe for the parser tests (no GPU): parses a JSON scene with the CPU builders and reports what Window
// would upload.  counts = {width, height, vertices, triangles, materials, lights, nodes, bvh depth};
// buffers (any may be NULL) receive the flat arrays in the wire format.
namespace glrt {
struct SceneProbe {
    static int run(const char *json, const char *bvh_kind, long long counts[8], float view[16], float proj[16], float lens[2], float *vert,
                   float *tri, float *mat, float *light, float *nodes) {
        Scene sc;
        if (bvh_kind && *bvh_kind) sc.setBvhBuilder(bvh_kind);
        sc.parse(json);
        const long long c[8] = {sc.width, sc.height, (long long)sc.vertices.size(), (long long)sc.triangles.size(),
                                (long long)sc.materials.size(), (long long)sc.lights.size(), (long long)sc.nodes.size(), sc.bvhDepth_};
        for (int i = 0; i < 8; i++) counts[i] = c[i];
        if (view) std::memcpy(view, sc.viewM, sizeof sc.viewM);
        if (proj) std::memcpy(proj, sc.projM, sizeof sc.projM);
        if (lens) { lens[0] = sc.apertureRadius; lens[1] = sc.focalLength; }
        if (vert && !sc.vertices.empty()) std::memcpy(vert, sc.vertices.data(), sc.vertices.size() * sizeof(Vertex));
        if (tri && !sc.triangles.empty()) std::memcpy(tri, sc.triangles.data(), sc.triangles.size() * sizeof(Triangle));
        if (mat && !sc.materials.empty()) std::memcpy(mat, sc.materials.data(), sc.materials.size() * sizeof(Material));
        if (light && !sc.lights.empty()) std::memcpy(light, sc.lights.data(), sc.lights.size() * sizeof(Triangle));
        if (nodes && !sc.nodes.empty()) std::memcpy(nodes, sc.nodes.data(), sc.nodes.size() * sizeof(BVHNode));
        return 0;
    }
};
}  // namespace glrt

// Volume block probe: enable = Scene::enableVolume before parse().  info = {number of volume blocks, 1 if the first block's files were loaded,
// nx, ny, nz}; bbox = the first block's {bboxMin, bboxMax}; density_max = u_densityMax Window would upload.
namespace glrt {
struct SceneVolumeProbe {
    static int run(const char *json, int enable, int info[5], float bbox[6], float *density_max) {
        Scene sc;
        sc.enableVolume(enable != 0);
        sc.parse(json);
        info[0] = (int)sc.volumeSpecs_.size();
        info[1] = sc.hasVolume_ ? 1 : 0;
        info[2] = sc.volDensity_.nx; info[3] = sc.volDensity_.ny; info[4] = sc.volDensity_.nz;
        if (!sc.volumeSpecs_.empty())
            for (int k = 0; k < 3; k++) { bbox[k] = sc.volumeSpecs_[0].bboxMin[k]; bbox[3 + k] = sc.volumeSpecs_[0].bboxMax[k]; }
        *density_max = sc.hasVolume_ ? sc.volDensity_.maxValue() : 0.0f;
        return 0;
    }
};
}  // namespace glrt

// Animation probe: parse the scene, then the animation file.  counts = {steps, shapes}; first_vertex (shapes + 1 values: the last is the vertex count), matrices
// (steps x shapes x 12), has_camera (steps) and cameras (steps x 34: view, proj, aperture, focal length; zeros without a camera) may each be NULL.
namespace glrt {
struct SceneAnimationProbe {
    static int run(const char *json, const char *animation, long long counts[2], long long *first_vertex, float *matrices, int *has_camera, float *cameras) {
        Scene sc;
        sc.parse(json);
        sc.parseAnimation(animation);
        const size_t n_shapes = sc.numShapes(), n_steps = sc.animation_.size();
        counts[0] = (long long)n_steps; counts[1] = (long long)n_shapes;
        if (first_vertex)
            for (size_t i = 0; i <= n_shapes; i++) first_vertex[i] = (long long)sc.shapeFirstVertex(i);
        for (size_t s = 0; s < n_steps; s++) {
            const Scene::AnimationStep &st = sc.animation_[s];
            if (matrices && n_shapes) std::memcpy(matrices + s * 12 * n_shapes, st.matrices.data(), 12 * n_shapes * sizeof(float));
            if (has_camera) has_camera[s] = st.hasCamera ? 1 : 0;
            if (cameras) {
                float *c = cameras + 34 * s;
                std::memset(c, 0, 34 * sizeof(float));
                if (st.hasCamera) { std::memcpy(c, st.viewM, 64); std::memcpy(c + 16, st.projM, 64); c[32] = st.apertureRadius; c[33] = st.focalLength; }
            }
        }
        return 0;
    }
};
}  // namespace glrt

// Morph probe: parse the scene, then the animation file.  counts = {steps, targets, vertices}; target_shape (targets), deltas (targets x vertices x 6) and weights
// (steps x targets) may each be NULL.
namespace glrt {
struct SceneMorphProbe {
    static int run(const char *json, const char *animation, long long counts[3], int *target_shape, float *deltas, float *weights) {
        Scene sc;
        sc.parse(json);
        sc.parseAnimation(animation);
        const size_t n_steps = sc.animation_.size(), n_targets = sc.numMorphTargets();
        counts[0] = (long long)n_steps; counts[1] = (long long)n_targets; counts[2] = (long long)sc.vertices.size();
        if (target_shape)
            for (size_t t = 0; t < n_targets; t++) target_shape[t] = (int)sc.morphShape_[t];
        if (deltas && !sc.morphDeltas_.empty()) std::memcpy(deltas, sc.morphDeltas_.data(), sc.morphDeltas_.size() * sizeof(float));
        if (weights && n_targets)
            for (size_t s = 0; s < n_steps; s++) std::memcpy(weights + s * n_targets, sc.animation_[s].weights.data(), n_targets * sizeof(float));
        return 0;
    }
};
}  // namespace glrt

// Sparse morph probe: as the morph probe for a file with "sparse_targets": true.  counts = {steps, targets, vertices, entries, sparse (0 / 1)}; target_shape
// (targets), offsets (targets + 1), vertex (entries), deltas (entries x 6) and weights (steps x targets) may each be NULL.
namespace glrt {
struct SceneMorphSparseProbe {
    static int run(const char *json, const char *animation, long long counts[5], int *target_shape, uint64_t *offsets, uint32_t *vertex, float *deltas, float *weights) {
        Scene sc;
        sc.parse(json);
        sc.parseAnimation(animation);
        const size_t n_steps = sc.animation_.size(), n_targets = sc.numMorphTargets(), nnz = sc.morphVertex_.size();
        counts[0] = (long long)n_steps; counts[1] = (long long)n_targets; counts[2] = (long long)sc.vertices.size();
        counts[3] = (long long)nnz; counts[4] = sc.morphSparse_ ? 1 : 0;
        if (target_shape)
            for (size_t t = 0; t < n_targets; t++) target_shape[t] = (int)sc.morphShape_[t];
        if (offsets && !sc.morphOffsets_.empty()) std::memcpy(offsets, sc.morphOffsets_.data(), sc.morphOffsets_.size() * sizeof(uint64_t));
        if (vertex && nnz) std::memcpy(vertex, sc.morphVertex_.data(), nnz * sizeof(uint32_t));
        if (deltas && nnz) std::memcpy(deltas, sc.morphSparseDeltas_.data(), nnz * 6 * sizeof(float));
        if (weights && n_targets)
            for (size_t s = 0; s < n_steps; s++) std::memcpy(weights + s * n_targets, sc.animation_[s].weights.data(), n_targets * sizeof(float));
        return 0;
    }
};
}  // namespace glrt

// Normals probe: what an animation file says about rebuilding normals.  out = {rebuild_normals (0 / 1), the topology flags}.
namespace glrt {
struct SceneNormalsProbe {
    static int run(const char *json, const char *animation, int out[2]) {
        Scene sc;
        sc.parse(json);
        sc.parseAnimation(animation);
        out[0] = sc.rebuildNormals_ ? 1 : 0;
        out[1] = (int)sc.normalFlags_;
        return 0;
    }
};
}  // namespace glrt

// Texture probe: parse with extensions on or off.  counts = {textures, materials}; per texture info[7k..] = {material, width, height, format, wrap, filter, texel
// bytes}; texels (may be NULL): the textures' texels one after the other, at most texel_cap bytes.
namespace glrt {
struct SceneTextureProbe {
    static int run(const char *json, int extensions, long long counts[2], int *info, unsigned char *texels, size_t texel_cap) {
        Scene sc;
        sc.enableExtensions(extensions != 0);
        sc.parse(json);
        counts[0] = (long long)sc.textures_.size();
        counts[1] = (long long)sc.materials.size();
        size_t at = 0;
        for (size_t k = 0; k < sc.textures_.size(); k++) {
            const Scene::TextureSpec &t = sc.textures_[k];
            if (info) {
                const int row[7] = {(int)t.material, t.image.width, t.image.height, t.format, t.wrap, t.filter, (int)t.image.texels.size()};
                std::memcpy(info + 7 * k, row, sizeof row);
            }
            if (texels && at + t.image.texels.size() <= texel_cap) std::memcpy(texels + at, t.image.texels.data(), t.image.texels.size());
            at += t.image.texels.size();
        }
        return 0;
    }
};
}  // namespace glrt

extern "C" GLRT_API int glrt_scene_texture_probe(const char *json, int extensions, long long counts[2], int *info, unsigned char *texels, size_t texel_cap) {
    return glrt::SceneTextureProbe::run(json, extensions, counts, info, texels, texel_cap);
}

// Emission-map probe: parse with extensions on or off.  Returns the number of emission maps; per map info[6k..] = {material, width, height, format, wrap, filter}.
namespace glrt {
struct SceneEmissionProbe {
    static int run(const char *json, int extensions, int *info, int cap) {
        Scene sc;
        sc.enableExtensions(extensions != 0);
        sc.parse(json);
        for (size_t k = 0; k < sc.emissionMaps_.size() && (int)k < cap; k++) {
            const Scene::TextureSpec &t = sc.emissionMaps_[k];
            const int row[6] = {(int)t.material, t.image.width, t.image.height, t.format, t.wrap, t.filter};
            if (info) std::memcpy(info + 6 * k, row, sizeof row);
        }
        return (int)sc.emissionMaps_.size();
    }
};
}  // namespace glrt

extern "C" GLRT_API int glrt_scene_emission_probe(const char *json, int extensions, int *info, int cap) {
    return glrt::SceneEmissionProbe::run(json, extensions, info, cap);
}

// Material-map probe: parse with extensions on or off.  Returns the number of maps; per map info[7k..] = {material, roughness (0 / 1), width, height, format,
// wrap, filter} and scale[k].
namespace glrt {
struct SceneMapProbe {
    static int run(const char *json, int extensions, int *info, float *scale, int cap) {
        Scene sc;
        sc.enableExtensions(extensions != 0);
        sc.parse(json);
        for (size_t k = 0; k < sc.maps_.size() && (int)k < cap; k++) {
            const Scene::MapSpec &t = sc.maps_[k];
            const int row[7] = {(int)t.material, t.roughness ? 1 : 0, t.image.width, t.image.height, t.format, t.wrap, t.filter};
            if (info) std::memcpy(info + 7 * k, row, sizeof row);
            if (scale) scale[k] = t.scale;
        }
        return (int)sc.maps_.size();
    }
};
}  // namespace glrt

extern "C" GLRT_API int glrt_scene_map_probe(const char *json, int extensions, int *info, float *scale, int cap) {
    return glrt::SceneMapProbe::run(json, extensions, info, scale, cap);
}

// Cutout probe: parse with extensions on or off.  Returns the number of cutouts; per cutout info[7k..] = {material, channel, width, height, format, wrap,
// filter} and cutoff[k].
namespace glrt {
struct SceneCutoutProbe {
    static int run(const char *json, int extensions, int *info, float *cutoff, int cap) {
        Scene sc;
        sc.enableExtensions(extensions != 0);
        sc.parse(json);
        for (size_t k = 0; k < sc.cutouts_.size() && (int)k < cap; k++) {
            const Scene::CutoutSpec &t = sc.cutouts_[k];
            const int row[7] = {(int)t.material, t.channel, t.image.width, t.image.height, t.format, t.wrap, t.filter};
            if (info) std::memcpy(info + 7 * k, row, sizeof row);
            if (cutoff) cutoff[k] = t.cutoff;
        }
        return (int)sc.cutouts_.size();
    }
};
}  // namespace glrt

extern "C" GLRT_API int glrt_scene_cutout_probe(const char *json, int extensions, int *info, float *cutoff, int cap) {
    return glrt::SceneCutoutProbe::run(json, extensions, info, cutoff, cap);
}

// Environment probe: parse with extensions on or off and an optional mode override (-1: none).  info = {present, mode, size, format, filter, latlong, texel
// bytes}; values = {scale[3], rotate_y, light_pick}; texels (may be NULL): the octahedral map, at most texel_cap bytes.
namespace glrt {
struct SceneEnvironmentProbe {
    static int run(const char *json, int extensions, int mode_override, int info[7], float values[5], unsigned char *texels, size_t texel_cap) {
        Scene sc;
        sc.enableExtensions(extensions != 0);
        sc.setEnvMode(mode_override);
        sc.parse(json);
        const Scene::EnvironmentSpec &e = sc.environment_;
        const int row[7] = {e.present ? 1 : 0, e.mode, e.size, e.format, e.filter, e.latlong ? 1 : 0, (int)e.texels.size()};
        std::memcpy(info, row, sizeof row);
        const float v[5] = {e.scale[0], e.scale[1], e.scale[2], e.rotateY, e.lightPick};
        std::memcpy(values, v, sizeof v);
        if (texels && e.texels.size() <= texel_cap) std::memcpy(texels, e.texels.data(), e.texels.size());
        return 0;
    }
};
}  // namespace glrt

extern "C" GLRT_API int glrt_scene_environment_probe(const char *json, int extensions, int mode_override, int info[7], float values[5], unsigned char *texels,
                                                     size_t texel_cap) {
    return glrt::SceneEnvironmentProbe::run(json, extensions, mode_override, info, values, texels, texel_cap);
}

extern "C" GLRT_API int glrt_scene_normals_probe(const char *json, const char *animation, int out[2]) { return glrt::SceneNormalsProbe::run(json, animation, out); }

extern "C" GLRT_API int glrt_scene_morph_sparse_probe(const char *json, const char *animation, long long counts[5], int *target_shape, uint64_t *offsets,
                                                      uint32_t *vertex, float *deltas, float *weights) {
    return glrt::SceneMorphSparseProbe::run(json, animation, counts, target_shape, offsets, vertex, deltas, weights);
}

extern "C" GLRT_API int glrt_scene_morph_probe(const char *json, const char *animation, long long counts[3], int *target_shape, float *deltas, float *weights) {
    return glrt::SceneMorphProbe::run(json, animation, counts, target_shape, deltas, weights);
}

extern "C" GLRT_API int glrt_scene_animation_probe(const char *json, const char *animation, long long counts[2], long long *first_vertex, float *matrices,
                                                   int *has_camera, float *cameras) {
    return glrt::SceneAnimationProbe::run(json, animation, counts, first_vertex, matrices, has_camera, cameras);
}

extern "C" GLRT_API int glrt_scene_volume_probe(const char *json, int enable, int info[5], float bbox[6], float *density_max) {
    return glrt::SceneVolumeProbe::run(json, enable, info, bbox, density_max);
}

extern "C" GLRT_API int glrt_scene_probe(const char *json, const char *bvh_kind, long long counts[8], float view[16], float proj[16],
                                         float lens[2], float *vert, float *tri, float *mat, float *light, float *nodes) {
    return glrt::SceneProbe::run(json, bvh_kind, counts, view, proj, lens, vert, tri, mat, light, nodes);
}
