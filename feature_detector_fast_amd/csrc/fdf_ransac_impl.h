// fdf_ransac_impl.h -- the file-local pieces that the estimators of fdf_ransac.hip and
// fdf_fundamental.hip share: what a correspondence is and how its coordinates become doubles.
// Device code only; every includer gets its own copy (an unnamed namespace), and includes
// fdf_common.h and fdf_kernels.h first.
#pragma once

namespace fdfk {

namespace {

constexpr double kRansacMinPivot = 0x1p-20;

struct Corr { double x, y, u, v; };

// The bits of a coordinate as a double: exact for both types.
__device__ __forceinline__ double coord(uint32_t bits, uint32_t coords) {
    return coords == kRansacF32 ? (double)__uint_as_float(bits) : (double)bits;
}

// Is query i (inside the frame's query range) a correspondence of the frame whose train range is
// `tr`?  Yes: *c holds it.  The match's index is compared with the range before t_coords is read.
__device__ __forceinline__ bool correspondence(const RansacParams& P, uint64_t i, IndexRange tr,
                                               Corr* c) {
    if (P.keep && P.keep[i] == 0) return false;
    const uint32_t j = P.matches[i].x;
    if (j == kMatchNone || j < tr.lo || j >= tr.hi) return false;
    const uint2 q = P.q_coords[i], t = P.t_coords[j];
    c->x = coord(q.x, P.coords);
    c->y = coord(q.y, P.coords);
    c->u = coord(t.x, P.coords);
    c->v = coord(t.y, P.coords);
    return true;
}

}  // namespace

}  // namespace fdfk
