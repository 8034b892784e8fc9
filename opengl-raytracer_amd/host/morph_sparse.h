// morph_sparse.h -- what glrt_deform_vertices_sparse (host/deform.cpp) and the device library (csrc/glrtx.hip: glrtx_upload_morph_targets_sparse,
// glrtx_debug_deform_sparse) share about a sparse morph-target set in its wire form (include/glrtx.h "Deforming", SPARSE TARGETS): the one check that decides
// what is refused, and the words of the refusal.  Plain C++, no dependency on either library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace glrt_detail {

constexpr int kMaxSparseTargets = 1024;  // GLRT_MAX_SPARSE_MORPH_TARGETS, GLRTX_MAX_SPARSE_MORPH_TARGETS

// Why a set is refused: the kind, and the target and the entry (counted inside the target) where it shows
struct SparseFault {
    enum Kind { kNone, kCount, kNullOffsets, kFirstOffset, kDecreasing, kTooMany, kNullArrays, kIndex, kOrder } kind = kNone;
    int target = 0;
    uint64_t entry = 0, a = 0, b = 0;
};

// offsets[n_targets + 1] with offsets[0] == 0, non-decreasing, nnz = offsets[n_targets] < 2^31; vertex[nnz] strictly ascending inside a target and < n_vert;
// deltas are not looked at.  n_targets == 0 needs no array at all.  Returns true for a set that goes through.
inline bool morph_sparse_check(const uint64_t *offsets, const uint32_t *vertex, const float *deltas, int n_targets, size_t n_vert, SparseFault &f) {
    f = SparseFault{};
    if (n_targets < 0 || n_targets > kMaxSparseTargets) { f.kind = SparseFault::kCount; return false; }
    if (n_targets == 0) return true;
    if (!offsets) { f.kind = SparseFault::kNullOffsets; return false; }
    if (offsets[0] != 0) { f.kind = SparseFault::kFirstOffset; f.a = offsets[0]; return false; }
    for (int k = 0; k < n_targets; k++)
        if (offsets[k + 1] < offsets[k]) { f.kind = SparseFault::kDecreasing; f.target = k; f.a = offsets[k]; f.b = offsets[k + 1]; return false; }
    const uint64_t nnz = offsets[n_targets];
    if (nnz >= ((uint64_t)1 << 31)) { f.kind = SparseFault::kTooMany; f.a = nnz; return false; }
    if (nnz > 0 && (!vertex || !deltas)) { f.kind = SparseFault::kNullArrays; return false; }
    for (int k = 0; k < n_targets; k++)
        for (uint64_t e = offsets[k]; e < offsets[k + 1]; e++) {
            if (vertex[e] >= n_vert) { f.kind = SparseFault::kIndex; f.target = k; f.entry = e - offsets[k]; f.a = vertex[e]; f.b = n_vert; return false; }
            if (e > offsets[k] && vertex[e] <= vertex[e - 1]) {
                f.kind = SparseFault::kOrder; f.target = k; f.entry = e - offsets[k]; f.a = vertex[e]; f.b = vertex[e - 1];
                return false;
            }
        }
    return true;
}

inline void morph_sparse_message(const SparseFault &f, int n_targets, char *buf, size_t n) {
    const unsigned long long a = f.a, b = f.b, e = f.entry;
    switch (f.kind) {
        case SparseFault::kNone: std::snprintf(buf, n, "no fault"); break;
        case SparseFault::kCount: std::snprintf(buf, n, "%d sparse morph targets (0 .. %d)", n_targets, kMaxSparseTargets); break;
        case SparseFault::kNullOffsets: std::snprintf(buf, n, "NULL offsets"); break;
        case SparseFault::kFirstOffset: std::snprintf(buf, n, "offsets[0] is %llu, not 0", a); break;
        case SparseFault::kDecreasing: std::snprintf(buf, n, "target %d: offsets decrease from %llu to %llu", f.target, a, b); break;
        case SparseFault::kTooMany: std::snprintf(buf, n, "%llu entries (at most 2^31 - 1)", a); break;
        case SparseFault::kNullArrays: std::snprintf(buf, n, "NULL vertex or deltas array with entries to read"); break;
        case SparseFault::kIndex: std::snprintf(buf, n, "target %d, entry %llu: vertex index %llu of %llu", f.target, e, a, b); break;
        case SparseFault::kOrder: std::snprintf(buf, n, "target %d, entry %llu: vertex index %llu after %llu, not strictly ascending", f.target, e, a, b); break;
    }
}

// glrt_morph_sparsify's rule: an entry is kept iff one of its six floats has a non-zero exponent field (a normal number, an Inf or a NaN)
inline bool morph_entry_kept(const float *d6) {
    for (int c = 0; c < 6; c++) {
        uint32_t u;
        __builtin_memcpy(&u, d6 + c, 4);
        if (u & 0x7F800000u) return true;
    }
    return false;
}

}  // namespace glrt_detail
