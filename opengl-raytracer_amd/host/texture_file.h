// texture_file.h -- the two image files a "texture" block may name (scene.h), read with own code, written from the file formats:
//   PPM, binary (P6), 8 bits a channel: "P6", width, height, maxval (255) as decimal text separated by whitespace, '#' comments to the end of a line
//        allowed in the header, ONE whitespace byte, then width*height RGB byte triples, rows from the TOP of the image down.
//   PFM: "PF" (three channels) or "Pf" (one, replicated to three), width, height, then a scale whose SIGN gives the byte order (negative: little-endian),
//        one whitespace byte, then width*height float32 pixels, rows from the BOTTOM of the image up.  Values are linear; the scale's magnitude is ignored.
// Both come back as RGBA texels with ROW 0 AT t = 0 -- the bottom row of the picture, OBJ's convention for vt (the top row of a PPM is t = 1): a PPM's rows are
// flipped, a PFM's are not.  Alpha is 255 / 1.0 (nothing reads it).
#pragma once
#include <string>
#include <vector>

#include "common.h"

namespace glrt {

struct TextureImage {
    int width = 0, height = 0;
    bool isFloat = false;              // PFM: 16 bytes a texel (float32 RGBA); PPM: 4 bytes a texel
    std::vector<unsigned char> texels;
};

// false + err on a missing file, an unknown magic, a maxval other than 255, dimensions outside 1 .. 16384 or a short file
GLRT_API bool readTextureFile(const std::string &path, TextureImage &out, std::string &err);

}  // namespace glrt
