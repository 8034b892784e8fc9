// texture_file.cpp -- readTextureFile (texture_file.h): binary PPM and PFM, own code.
#include "texture_file.h"

#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

namespace glrt {
namespace {

// the next whitespace-separated token of a PNM header at `at`, '#' comments skipped; "" at the end of the data
std::string token(const std::string &s, size_t &at) {
    for (;;) {
        while (at < s.size() && std::isspace((unsigned char)s[at])) at++;
        if (at < s.size() && s[at] == '#') { while (at < s.size() && s[at] != '\n') at++; continue; }
        break;
    }
    const size_t b = at;
    while (at < s.size() && !std::isspace((unsigned char)s[at])) at++;
    return s.substr(b, at - b);
}

bool dimension(const std::string &t, int &out) {
    char *end = nullptr;
    const long v = std::strtol(t.c_str(), &end, 10);
    if (t.empty() || *end != '\0' || v < 1 || v > 16384) return false;
    out = (int)v;
    return true;
}

}  // namespace

bool readTextureFile(const std::string &path, TextureImage &out, std::string &err) {
    std::ifstream f(path.c_str(), std::ios::in | std::ios::binary);
    if (f.fail()) { err = "cannot open " + path; return false; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string s = ss.str();
    size_t at = 0;
    const std::string magic = token(s, at);
    if (magic != "P6" && magic != "PF" && magic != "Pf") { err = path + ": neither a binary PPM (P6) nor a PFM (PF / Pf)"; return false; }
    int w = 0, h = 0;
    if (!dimension(token(s, at), w) || !dimension(token(s, at), h)) { err = path + ": width and height must be 1 .. 16384"; return false; }
    const std::string third = token(s, at);
    if (at >= s.size()) { err = path + ": no pixel data"; return false; }
    at++;  // the one whitespace byte behind the header
    out.width = w; out.height = h;
    const size_t n = (size_t)w * (size_t)h;
    if (magic == "P6") {
        if (third != "255") { err = path + ": maxval " + third + " (only 8-bit PPM, maxval 255)"; return false; }
        if (s.size() - at < 3 * n) { err = path + ": the file ends before its " + std::to_string(n) + " pixels do"; return false; }
        out.isFloat = false;
        out.texels.assign(4 * n, 255);
        for (int y = 0; y < h; y++) {  // file row y (from the top) is texture row h - 1 - y
            const unsigned char *src = (const unsigned char *)s.data() + at + 3 * (size_t)y * w;
            unsigned char *dst = out.texels.data() + 4 * (size_t)(h - 1 - y) * w;
            for (int x = 0; x < w; x++) { dst[4 * x] = src[3 * x]; dst[4 * x + 1] = src[3 * x + 1]; dst[4 * x + 2] = src[3 * x + 2]; }
        }
        return true;
    }
    char *end = nullptr;
    const double scale = std::strtod(third.c_str(), &end);
    if (third.empty() || *end != '\0' || scale == 0.0) { err = path + ": bad PFM scale '" + third + "'"; return false; }
    const int ch = magic == "PF" ? 3 : 1;
    if (s.size() - at < 4 * n * ch) { err = path + ": the file ends before its " + std::to_string(n) + " pixels do"; return false; }
    const bool little = scale < 0.0;
    out.isFloat = true;
    out.texels.assign(16 * n, 0);
    const float one = 1.0f;
    for (size_t p = 0; p < n; p++) {  // rows already run from the bottom up
        for (int c = 0; c < 3; c++) {
            const unsigned char *b = (const unsigned char *)s.data() + at + 4 * (p * ch + (ch == 3 ? c : 0));
            const uint32_t u = little ? ((uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24)
                                      : ((uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24);
            std::memcpy(out.texels.data() + 16 * p + 4 * c, &u, 4);
        }
        std::memcpy(out.texels.data() + 16 * p + 12, &one, 4);
    }
    return true;
}

}  // namespace glrt
