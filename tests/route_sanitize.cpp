// Stand-alone driver for AddressSanitizer / UBSan: the route statement (host/route_statement.h through glrt_launch_route, host/route.cpp) over the whole
// enumeration of tests/golden/route_matrix.txt and over hostile arguments.  tests/test_route_host.py builds and runs it.
#include <climits>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "glrt_host.h"

static int g_failed = 0;
static void check(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); g_failed++; }
}

int main() {
    const int exts[4] = {0, 2, 4, 6}, depths[4] = {2, 256, 2, 2}, samples[4] = {1, 1, 1 << 16, 1 << 20};
    long launches = 0, refusals = 0;
    char msg[320];
    glrt_route r;
    for (int kind = GLRT_ROUTE_ORDINARY; kind <= GLRT_ROUTE_CASCADES; kind++)
        for (int bits = 0; bits < 1 << 11; bits++)  // tex, maps, cut, emit, env, vine, the switches, spheres, have_volume, and a set of 70000 textures
            for (int variant = 0; variant < 3; variant++)
                for (int e = 0; e < 4; e++)
                    for (int pc = 0; pc < 4; pc++) {
                        const glrt_route_state s{variant,      exts[e],      bits & 1 ? 3 : 0, bits & 2 ? (bits & 1024 ? 70000 : 2) : 0, bits & 4 ? 2 : 0, bits >> 3 & 1, bits >> 4 & 1,
                                                 bits >> 5 & 1, bits >> 6 & 1, bits >> 7 & 1,    bits >> 8 & 1, bits >> 9 & 1, depths[pc], samples[pc]};
                        const int rc = glrt_launch_route(&s, kind, &r, msg, sizeof msg);
                        check(rc == GLRT_HOST_OK || rc == GLRT_HOST_EINVAL, "a route or a refusal");
                        check((rc == GLRT_HOST_OK) == (msg[0] == 0) && (rc == GLRT_HOST_OK) == (r.kernel[0] != 0), "a kernel's name or a message, never both");
                        check(std::strlen(msg) < sizeof msg - 1 && std::strlen(r.kernel) < sizeof r.kernel - 1, "nothing is cut short");
                        check(r.family == r.variant_last && r.family >= 0 && r.family <= 2 && (r.fallback_last & ~7) == 0, "ranges");
                        (rc == GLRT_HOST_OK ? launches : refusals)++;
                    }
    check(launches > 0 && refusals > 0, "both happen");
    // hostile arguments: parameters at the ends of int, unknown flag bits, a variant that does not exist, tiny buffers, NULLs
    const int ends[6] = {INT_MIN, -1, 0, 255, 256, INT_MAX};
    for (int kind = 0; kind < 6; kind++)
        for (int d : ends)
            for (int n : ends)
                for (int v : {INT_MIN, -1, 3, INT_MAX}) {
                    const glrt_route_state s{v, (int)0x80000007, INT_MAX, INT_MAX, INT_MIN, 7, -1, 2, 0, 0, INT_MIN, INT_MAX, d, n};
                    char tiny[5];
                    const int rc = glrt_launch_route(&s, kind, &r, tiny, sizeof tiny);
                    check(rc == GLRT_HOST_OK || (rc == GLRT_HOST_EINVAL && std::strlen(tiny) == 4), "hostile fields");
                }
    const glrt_route_state plain{2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 1};
    check(glrt_launch_route(nullptr, 0, &r, msg, sizeof msg) == GLRT_HOST_EINDEX && glrt_launch_route(&plain, 0, nullptr, msg, sizeof msg) == GLRT_HOST_EINDEX, "NULLs");
    check(glrt_launch_route(&plain, 6, &r, msg, sizeof msg) == GLRT_HOST_EINDEX && glrt_launch_route(&plain, INT_MIN, &r, nullptr, 0) == GLRT_HOST_EINDEX, "no such kind");
    check(glrt_launch_route(&plain, 0, &r, nullptr, 0) == GLRT_HOST_OK && std::strcmp(r.kernel, "pt_render_wgwf") == 0 && r.family == 2, "no message buffer");
    check(glrt_launch_route(&plain, 0, &r, msg, 0) == GLRT_HOST_OK && glrt_launch_route(&plain, 0, &r, nullptr, 99) == GLRT_HOST_OK, "half a message buffer");
    if (g_failed) return 1;
    std::printf("route_sanitize ok: %ld launches, %ld refusals\n", launches, refusals);
    return 0;
}
