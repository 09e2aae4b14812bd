// irbpp_amd/csrc/irbpp_binstate.h compiled for the host (tests/test_bin_state_cpu.py): the segment table of a bin's state and the
// key routines are plain functions, so the program needs no device.  One request per line on standard input:
//     table Ax Ay step R S K wide log_cap      -> "n bytes_per_bin", then one line "name row_bytes bytes offset in_fork" per segment, then
//                                                 "geometry KEY" (hex)
//     seqkey n_traj length id id ...           -> "key KEY": bin_sequences_key of the ids
//     shapeskey index                          -> "key KEY": bin_shapes_key of a fixed two-shape, two-rotation table set whose pool
//                                                 value `index` (counted through height_top, height_bottom, mask_top, mask_bottom)
//                                                 is changed when index >= 0
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
struct uint2 { unsigned x, y; };

#include "../../irbpp_amd/csrc/irbpp_binstate.h"

using namespace irbpp;

int main() {
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "table")) {
            int Ax, Ay, step, R, S, K, wide, log_cap;
            if (scanf("%d %d %d %d %d %d %d %d", &Ax, &Ay, &step, &R, &S, &K, &wide, &log_cap) != 8) return 2;
            Params P{};
            P.Ax = Ax; P.Ay = Ay; P.step = step; P.R = R; P.S = S; P.K = K;
            P.Hx = Ax * step; P.Hy = Ay * step; P.Hc = P.Hx * P.Hy; P.AC = Ax * Ay;
            P.wide = wide; P.vrow = wide ? 32 : 16;                       // (irbpp_create)
            const BinSegTable t = bin_segments(P, log_cap);
            printf("%d %d\n", t.n, t.bytes_per_bin);
            for (int i = 0; i < t.n; ++i)
                printf("%s %d %d %d %d\n", bin_array_name(t.seg[i].array), t.seg[i].row_bytes, t.seg[i].bytes, t.seg[i].offset,
                       bin_array_in_fork(t.seg[i].array) ? 1 : 0);
            printf("geometry %016llx\n", (unsigned long long)bin_geometry_key(P, log_cap));
        } else if (!strcmp(cmd, "seqkey")) {
            int n_traj, length;
            if (scanf("%d %d", &n_traj, &length) != 2 || n_traj < 1 || length < 1 || n_traj * length > 4096) return 2;
            std::vector<int32_t> ids((size_t)n_traj * length);
            for (auto& v : ids) if (scanf("%d", &v) != 1) return 2;
            printf("key %016llx\n", (unsigned long long)bin_sequences_key(ids.data(), n_traj, length));
        } else if (!strcmp(cmd, "shapeskey")) {
            int index;
            if (scanf("%d", &index) != 1) return 2;
            const int n = 2, R = 2, cells = 6;                             // every (shape, rotation) a 2 x 3 table
            std::vector<double> ext(n * R * 3), vol(n), pool[4];
            std::vector<int32_t> dims(n * R * 2);
            std::vector<int64_t> offs(n * R);
            for (int i = 0; i < n * R; ++i) { dims[2 * i] = 2; dims[2 * i + 1] = 3; offs[i] = (int64_t)i * cells; }
            for (size_t i = 0; i < ext.size(); ++i) ext[i] = 0.02 + 0.01 * (double)i;
            for (int i = 0; i < n; ++i) vol[i] = 1e-5 * (i + 1);
            for (int p = 0; p < 4; ++p)
                for (int i = 0; i < n * R * cells; ++i) pool[p].push_back(p < 2 ? 0.01 * (i % 5) + 0.001 * p : 1.0);
            const int per = n * R * cells;
            if (index >= 4 * per) return 2;
            if (index >= 0) pool[index / per][index % per] += 0.5;
            printf("key %016llx\n", (unsigned long long)bin_shapes_key(n, R, ext.data(), vol.data(), dims.data(), offs.data(), per,
                                                                       pool[0].data(), pool[1].data(), pool[2].data(), pool[3].data()));
        } else {
            return 2;
        }
    }
    return 0;
}
