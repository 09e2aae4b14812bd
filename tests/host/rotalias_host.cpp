// rotalias_host.cpp -- irbpp_amd/csrc/irbpp_rotalias.h (plain C++: which rotations of a shape have bit-identical observation
// inputs) for the host.  Two uses: tests/test_rot_alias_host.py loads it as a shared library and calls host_rot_aliases on
// tables it builds in numpy; built as a program, main() runs the same hand-made cases on its own (that is the form to build
// with -fsanitize=address,undefined).
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../irbpp_amd/csrc/irbpp_rotalias.h"

using irbpp::RotView;

// One shape: R rotations, tables [fx][fy] at offsets[r] of the two pools.  sizes = [R][5]: fx, fy, ax, ay, has_out.
extern "C" void host_rot_aliases(int R, const int32_t* sizes, const double* ext_z_r, const int64_t* offsets,
                                 const double* mask_bottom, const double* height_bottom, int32_t* alias_out) {
    std::vector<RotView> v((size_t)R);
    for (int r = 0; r < R; ++r)
        v[r] = RotView{sizes[r * 5], sizes[r * 5 + 1], sizes[r * 5 + 2], sizes[r * 5 + 3], sizes[r * 5 + 4], ext_z_r[r],
                       mask_bottom + offsets[r], height_bottom + offsets[r]};
    irbpp::rot_aliases(v.data(), R, alias_out);
}

namespace {

struct Rot {
    int fx, fy;
    double ext_z_r;
    std::vector<double> mask, bottom;
};

Rot solid(int fx, int fy, double ez) { return Rot{fx, fy, ez, std::vector<double>((size_t)fx * fy, 1.0), std::vector<double>((size_t)fx * fy, 0.0)}; }

std::vector<int32_t> aliases_of(const std::vector<Rot>& rots) {
    std::vector<RotView> v;
    for (const Rot& q : rots) {
        int has_out = 0;
        for (double m : q.mask) has_out |= m == 0.0;
        v.push_back(RotView{q.fx, q.fy, (q.fx + 1) / 2, (q.fy + 1) / 2, has_out, q.ext_z_r, q.mask.data(), q.bottom.data()});
    }
    std::vector<int32_t> a(rots.size());
    irbpp::rot_aliases(v.data(), (int)rots.size(), a.data());
    return a;
}

int failures = 0;
void expect(const char* what, const std::vector<int32_t>& got, const std::vector<int32_t>& want) {
    if (got == want) return;
    ++failures;
    printf("FAIL %s: got", what);
    for (int32_t g : got) printf(" %d", g);
    printf("\n");
}

}  // namespace

int main() {
    // a cube: all four rotations are one
    expect("cube", aliases_of({solid(4, 4, 0.04), solid(4, 4, 0.04), solid(4, 4, 0.04), solid(4, 4, 0.04)}), {0, 0, 0, 0});
    // a 1 x 2 bar: r and r + 2
    expect("bar", aliases_of({solid(4, 8, 0.04), solid(8, 4, 0.04), solid(4, 8, 0.04), solid(8, 4, 0.04)}), {0, 1, 0, 1});
    // an L-tromino: the missing corner is somewhere else in every rotation
    {
        std::vector<Rot> l;
        for (int k = 0; k < 4; ++k) {
            Rot q = solid(2, 2, 0.04);
            q.mask[k] = 0.0;
            l.push_back(q);
        }
        expect("L", aliases_of(l), {0, 1, 2, 3});
    }
    {   // only ext_z_r differs
        Rot a = solid(3, 3, 0.04), b = solid(3, 3, 0.05);
        expect("ext_z_r", aliases_of({a, b}), {0, 1});
    }
    {   // one ulp in one bottom height
        Rot a = solid(3, 3, 0.04), b = a;
        a.bottom[4] = 0.01;
        b.bottom[4] = nextafter(0.01, 1.0);
        expect("ulp", aliases_of({a, b}), {0, 1});
        b.bottom[4] = 0.01;
        expect("no ulp", aliases_of({a, b}), {0, 0});
        a.bottom[4] = 0.0;                           // +0 and -0 are different bit patterns
        b.bottom[4] = -0.0;
        expect("signed zero", aliases_of({a, b}), {0, 1});
    }
    {   // a masked-out cell that moved; and a bottom height under a masked-out cell, which nobody reads
        Rot a = solid(3, 3, 0.04), b = a, c = a;
        a.mask[0] = 0.0;
        b.mask[8] = 0.0;
        c.mask[0] = 0.0;
        c.bottom[0] = 7.0;
        expect("moved hole", aliases_of({a, b, c}), {0, 1, 0});
    }
    printf(failures ? "rotalias_host: %d failures\n" : "rotalias_host: ok\n", failures);
    return failures ? 1 : 0;
}
