// volume.h -- Mitsuba-style VOL grid files (version 3, float32), the format the reference's "media" material names
// (scene.cpp:174-214).  Own reader and writer, written from the file format:
//   bytes 0-2 "VOL", byte 3 version (3), int32 encoding (1 = float32), int32 xres, yres, zres, channels,
//   six float32 bbox values (min x y z, max x y z), then xres*yres*zres*channels float32, channels fastest, then x, y, z.
// All little-endian.
#pragma once
#include <string>
#include <vector>

#include "common.h"

namespace glrt {

struct VolumeGrid {
    int nx = 0, ny = 0, nz = 0, channels = 0;
    float bboxMin[3] = {0.f, 0.f, 0.f}, bboxMax[3] = {0.f, 0.f, 0.f};  // the file's own header (the scene's JSON bbox is the one rendered)
    std::vector<float> data;                                           // nx * ny * nz * channels
    // What the reference uploads (scene.cpp:186-188): glTexSubImage3D with GL_RED reads the FIRST nx*ny*nz floats, whatever the channel count.
    const float *texels() const { return data.data(); }
    // Volume::maxValue: the largest value of the whole file, every channel included (u_densityMax).
    float maxValue() const;
};

// false + err on a missing file, a bad magic, a version other than 3, an encoding other than float32, bad dimensions or a short file.
GLRT_API bool readVol(const std::string &path, VolumeGrid &out, std::string &err);
GLRT_API bool writeVol(const std::string &path, const VolumeGrid &g, std::string &err);

}  // namespace glrt
