// irbpp_rotalias.h -- which rotations of one shape have bit-identical observation inputs (plain C++, host only).
//
// The location observation of an item is built rotation by rotation (posZmap, naiveMask, level images, borders, vertex
// bits), and depends on a rotation only through its footprint sizes fx, fy, ax, ay, its bottom table (the masked-in cells
// and their heightMapB; has_out says whether a masked-out cell exists) and ext_z_r.  Two rotations that agree in all of
// these BIT FOR BIT produce identical observations on every heightmap, so the later one can reuse the earlier one's.
// The top table, the raw extents, the centre of mass and the volume take no part: they are used only when an action is
// applied, and that always uses the real rotation.
#pragma once
#include <stdint.h>
#include <string.h>

namespace irbpp {

struct RotView {
    int32_t fx, fy;                 // footprint in heightmap cells
    int32_t ax, ay;                 // footprint in action cells
    int32_t has_out;                // some cell of the bottom table is masked out
    double ext_z_r;                 // round(extents, 6)[2]
    const double* mask_bottom;      // [fx][fy], 0 = masked out
    const double* height_bottom;    // [fx][fy], read only where masked in
};

inline bool rot_same_bits(double a, double b) {
    uint64_t ua, ub;
    memcpy(&ua, &a, 8);
    memcpy(&ub, &b, 8);
    return ua == ub;
}

// true iff the two rotations' observation inputs are bit-identical
inline bool rot_same_observation(const RotView& a, const RotView& b) {
    if (a.fx != b.fx || a.fy != b.fy || a.ax != b.ax || a.ay != b.ay || a.has_out != b.has_out) return false;
    if (!rot_same_bits(a.ext_z_r, b.ext_z_r)) return false;
    const int64_t n = (int64_t)a.fx * a.fy;
    for (int64_t e = 0; e < n; ++e) {
        const bool in_a = a.mask_bottom[e] != 0.0, in_b = b.mask_bottom[e] != 0.0;
        if (in_a != in_b) return false;
        if (in_a && !rot_same_bits(a.height_bottom[e], b.height_bottom[e])) return false;
    }
    return true;
}

// alias[r] = the smallest c <= r whose observation inputs equal those of r (alias[r] == r: r is canonical)
inline void rot_aliases(const RotView* rots, int R, int32_t* alias) {
    for (int r = 0; r < R; ++r) {
        alias[r] = r;
        for (int c = 0; c < r; ++c)
            if (alias[c] == c && rot_same_observation(rots[c], rots[r])) { alias[r] = c; break; }
    }
}

}  // namespace irbpp
