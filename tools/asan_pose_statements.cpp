// The CPU statements of the pose kernels under AddressSanitizer and UBSan: a stand-alone program, host code only, no GPU and nothing loaded into Python.
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Iinclude -Iopengl-raytracer_amd/host
//         tools/asan_pose_statements.cpp opengl-raytracer_amd/host/deform.cpp -o asan_pose_statements       (one line), then ./asan_pose_statements
//
// glrt_skin_vertices, glrt_deform_vertices and glrt_deform_vertices_sparse on exactly sized heap buffers: 0, 1 and 65 vertices, matrices and dual quaternions,
// 0 and 3 targets (the middle one inactive), the sparse set made by glrt_morph_sparsify.  Also checks what the shared skinning stage promises: with matrices and
// no targets the three statements give the same bits.  Exit status 0 and "ok" when nothing was reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "glrt_host.h"

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) { return a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(float)); }

int main() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    const int n_bones = 5;
    int runs = 0;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)65})
        for (int mode : {0, 1})
            for (int n_targets : {0, 3}) {
                std::vector<float> rest(15 * n), weights(4 * n), data((size_t)n_bones * (mode ? 8 : 12)), deltas((size_t)n_targets * n * 6), mw(n_targets);
                std::vector<int32_t> bones(4 * n);
                for (float &x : rest) x = u(rng);
                for (float &x : weights) x = 0.25f + 0.1f * u(rng);
                for (float &x : data) x = u(rng);
                for (float &x : deltas) x = 0.05f * u(rng);
                for (int32_t &b : bones) b = (int32_t)(rng() % n_bones);
                if (n_targets) { mw[0] = 0.7f; mw[1] = 0.0f; mw[2] = -0.4f; }
                std::vector<float> dense(15 * n), sparse(15 * n), skinned(15 * n);
                if (glrt_deform_vertices(rest.data(), n, bones.data(), weights.data(), data.data(), n_bones, mode, n_targets ? deltas.data() : nullptr,
                                         n_targets ? mw.data() : nullptr, n_targets, dense.data()) != GLRT_HOST_OK) return 1;
                std::vector<uint64_t> offsets(n_targets + 1);
                if (glrt_morph_sparsify(deltas.data(), n_targets, n, offsets.data(), nullptr, nullptr) != GLRT_HOST_OK) return 2;
                std::vector<uint32_t> vertex(offsets[n_targets]);
                std::vector<float> sd(6 * (size_t)offsets[n_targets]);
                if (glrt_morph_sparsify(deltas.data(), n_targets, n, offsets.data(), vertex.data(), sd.data()) != GLRT_HOST_OK) return 3;
                if (glrt_deform_vertices_sparse(rest.data(), n, bones.data(), weights.data(), data.data(), n_bones, mode, offsets.data(), vertex.data(), sd.data(),
                                                n_targets ? mw.data() : nullptr, n_targets, sparse.data()) != GLRT_HOST_OK) return 4;
                if (!same_bits(dense, sparse)) return 5;  // (every delta here is kept by the sparsifier)
                if (mode == 0) {
                    if (glrt_skin_vertices(rest.data(), n, bones.data(), weights.data(), data.data(), n_bones, skinned.data()) != GLRT_HOST_OK) return 6;
                    if (n_targets == 0 && !same_bits(dense, skinned)) return 7;
                }
                // the refusals read nothing they should not: a bone index out of range, a NULL output
                if (n > 0) {
                    bones[4 * n - 1] = n_bones;
                    if (glrt_skin_vertices(rest.data(), n, bones.data(), weights.data(), data.data(), n_bones, skinned.data()) != GLRT_HOST_EINVAL) return 8;
                    bones[4 * n - 1] = 0;
                    if (glrt_deform_vertices(rest.data(), n, bones.data(), weights.data(), data.data(), n_bones, mode, nullptr, nullptr, 0, nullptr) != GLRT_HOST_EINVAL) return 9;
                }
                runs++;
            }
    std::printf("ok: %d cases\n", runs);
    return 0;
}
