// volume.cpp -- VOL grid files (volume.h).
#include "volume.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>

namespace glrt {

float VolumeGrid::maxValue() const {
    float m = 0.0f;
    bool first = true;
    for (float v : data) {
        if (first || v > m) m = v;
        first = false;
    }
    return m;
}

namespace {
int32_t rd_i32(const unsigned char *p) { int32_t v; std::memcpy(&v, p, 4); return v; }  // (hosts are little-endian, as the format)
float rd_f32(const unsigned char *p) { float v; std::memcpy(&v, p, 4); return v; }
}  // namespace

bool readVol(const std::string &path, VolumeGrid &out, std::string &err) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { err = "cannot open " + path; return false; }
    const std::vector<unsigned char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    constexpr size_t kHeader = 48;
    if (raw.size() < kHeader || std::memcmp(raw.data(), "VOL", 3) != 0) { err = path + ": not a VOL file"; return false; }
    if (raw[3] != 3) { err = path + ": VOL version " + std::to_string(raw[3]) + ", only 3 is supported"; return false; }
    const int32_t enc = rd_i32(&raw[4]);
    if (enc != 1) { err = path + ": VOL encoding " + std::to_string(enc) + ", only 1 (float32) is supported"; return false; }
    const int32_t nx = rd_i32(&raw[8]), ny = rd_i32(&raw[12]), nz = rd_i32(&raw[16]), nc = rd_i32(&raw[20]);
    if (nx <= 0 || ny <= 0 || nz <= 0 || nc <= 0 || (long long)nx * ny * nz * nc > (1ll << 31)) {
        err = path + ": bad VOL dimensions " + std::to_string(nx) + "x" + std::to_string(ny) + "x" + std::to_string(nz) + "x" + std::to_string(nc);
        return false;
    }
    const size_t n = (size_t)nx * ny * nz * nc;
    if (raw.size() < kHeader + 4 * n) { err = path + ": VOL header does not match the file size"; return false; }
    out.nx = nx; out.ny = ny; out.nz = nz; out.channels = nc;
    for (int k = 0; k < 3; k++) { out.bboxMin[k] = rd_f32(&raw[24 + 4 * k]); out.bboxMax[k] = rd_f32(&raw[36 + 4 * k]); }
    out.data.resize(n);
    std::memcpy(out.data.data(), &raw[kHeader], 4 * n);
    return true;
}

bool writeVol(const std::string &path, const VolumeGrid &g, std::string &err) {
    const size_t n = (size_t)g.nx * g.ny * g.nz * g.channels;
    if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0 || g.channels <= 0 || g.data.size() != n) { err = "writeVol: grid shape and data disagree"; return false; }
    std::ofstream f(path, std::ios::binary);
    if (!f) { err = "cannot write " + path; return false; }
    unsigned char hdr[48] = {'V', 'O', 'L', 3};
    const int32_t ints[5] = {1, g.nx, g.ny, g.nz, g.channels};
    std::memcpy(hdr + 4, ints, sizeof ints);
    std::memcpy(hdr + 24, g.bboxMin, 12);
    std::memcpy(hdr + 36, g.bboxMax, 12);
    f.write(reinterpret_cast<const char *>(hdr), sizeof hdr);
    f.write(reinterpret_cast<const char *>(g.data.data()), (std::streamsize)(4 * n));
    if (!f) { err = "short write to " + path; return false; }
    return true;
}

}  // namespace glrt

// ---------------------------------------------------------------------------------------------- test hooks
// dims = {nx, ny, nz, channels}, bbox = {min xyz, max xyz}; data (may be NULL) receives min(capacity, size) floats.  Returns 0, or -1 with
// the reader's message in err (err_cap bytes).
extern "C" GLRT_API int glrt_vol_read(const char *path, int dims[4], float bbox[6], float *data, size_t capacity, char *err, size_t err_cap) {
    glrt::VolumeGrid g;
    std::string e;
    if (!glrt::readVol(path, g, e)) {
        if (err && err_cap) { std::strncpy(err, e.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
        return -1;
    }
    dims[0] = g.nx; dims[1] = g.ny; dims[2] = g.nz; dims[3] = g.channels;
    for (int k = 0; k < 3; k++) { bbox[k] = g.bboxMin[k]; bbox[3 + k] = g.bboxMax[k]; }
    if (data) std::memcpy(data, g.data.data(), 4 * std::min(capacity, g.data.size()));
    return 0;
}
extern "C" GLRT_API int glrt_vol_write(const char *path, const int dims[4], const float bbox[6], const float *data) {
    glrt::VolumeGrid g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2]; g.channels = dims[3];
    for (int k = 0; k < 3; k++) { g.bboxMin[k] = bbox[k]; g.bboxMax[k] = bbox[3 + k]; }
    if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0 || g.channels <= 0) return -1;
    g.data.assign(data, data + (size_t)g.nx * g.ny * g.nz * g.channels);
    std::string e;
    return glrt::writeVol(path, g, e) ? 0 : -1;
}
