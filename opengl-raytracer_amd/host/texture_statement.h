// texture_statement.h -- the CPU statement of one texture lookup and of one texel decode (host/texture.cpp), for the statements that read a map through them
// (host/environment.cpp).  Internal to the host library.  The caller holds a FlushDenormals and has checked the descriptor (texture_set_error).
#pragma once
#include "texture_set.h"

namespace glrt_detail {

void texture_lookup_one(const TexRecord &d, const unsigned char *texels, float s, float t, float rgb[3]);
void texture_texel_one(const TexRecord &d, const unsigned char *texels, int ix, int iy, float rgb[3]);
float texture_channel_one(const TexRecord &d, const unsigned char *texels, int channel, float s, float t);  // "Cutouts": one channel, 0 .. 3 (host/query.cpp's cutout walker)

}  // namespace glrt_detail
