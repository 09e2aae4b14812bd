// irbpp_amd/csrc/irbpp_plan.h compiled for the host (tests/test_launch_plan_host.py): the launch plan of a transition is a pure
// function, so the program needs no device.  It reads one request per line from standard input,
//     GEOMETRY N K stability tuning mode n key listed registered_obs heavy_turn item_order
// and prints the geometry's LDS sizes (from irbpp::layout_lds, which is not under test), the plan's launches as lines of
// "kernel grid block lds mode" and the plan's facts.  GEOMETRY: s1 .. s5 = spec_params(SPEC_KEYS[1..5]); the others are filled
// in by hand below; GEOMETRY@BYTES overrides Params::lds_bytes (the tile sizes the chain build's limit lies between).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __host__
#define __device__
#define __forceinline__ inline
struct uint2 { unsigned x, y; };

#include "../../irbpp_amd/csrc/irbpp_plan.h"

using namespace irbpp;

static bool geometry(const char* name, Params& P) {
    if (name[0] == 's' && name[1] >= '1' && name[1] <= '5' && name[2] == 0) { P = spec_params(SPEC_KEYS[name[1] - '0']); return true; }
    // 12 x 12 action cells: no row of SPEC_KEYS -- free-form footprints, solid boxes, lattice footprints of 4 x 4 cells
    if (!strcmp(name, "generic12")) { P = spec_params(SpecKey{12, 12, 2, 4, 500, 0, 0, 0}); return true; }
    if (!strcmp(name, "box12")) { P = spec_params(SpecKey{12, 12, 2, 2, 500, 0, 1, 0}); return true; }
    if (!strcmp(name, "lattice12")) { P = spec_params(SpecKey{12, 12, 2, 4, 500, 4, 0, 0x0F}); return true; }
    if (!strcmp(name, "wide20")) {      // 20 x 20 action cells: the capacity path (as irbpp_create sets it up)
        P = spec_params(SpecKey{16, 16, 2, 4, 500, 0, 0, 0});
        P.Ax = P.Ay = 20; P.Hx = P.Hy = 40; P.Hc = 1600; P.AC = 400;
        P.wide = 1; P.vrow = 32;
        return true;
    }
    return false;
}

int main() {
    char name[32];
    int N, K, stability, tuning, mode, n, key, listed, registered, turn, item_order;
    while (scanf("%31s %d %d %d %d %d %d %d %d %d %d %d", name, &N, &K, &stability, &tuning, &mode, &n, &key, &listed, &registered, &turn,
                 &item_order) == 12) {
        Params P;
        int lds_override = 0;
        if (char* at = strchr(name, '@')) { *at = 0; lds_override = atoi(at + 1); }
        if (!geometry(name, P) || N < 1 || n < 1 || n > N) { printf("bad request\n"); return 2; }
        P.N = N;
        P.K = K;
        P.stability = stability;
        P.heavy_cap = N >= 64 ? N / 8 : 0;              // (irbpp_create)
        if (lds_override > 0) P.lds_bytes = lds_override;
        P.obs_len0 = K > 1 ? K + P.Hc : P.obs_len1;
        const Plan plan = plan_transition(P, tuning, mode, n, key, listed != 0, registered != 0, turn, item_order != 0);
        if (plan.n_launches < 0 || plan.n_launches > (int)(sizeof plan.launch / sizeof plan.launch[0])) { printf("bad plan\n"); return 3; }
        printf("layout lds=%d full=%d emit=%d heavy_cap=%d\n", P.lds_bytes, P.lds_bytes_full, P.emit_lds_bytes, P.heavy_cap);
        for (int i = 0; i < plan.n_launches; ++i) {
            const Launch& l = plan.launch[i];
            printf("%s %d %d %d %d\n", kernel_info(l.kernel).name, l.grid, l.block, l.lds, l.mode);
        }
        printf("facts use_order=%d heavy_first=%d heavy_turn=%d inline_polygon=%d obs_rows=%d\n", plan.use_order, plan.heavy_first,
               plan.heavy_turn, plan.inline_polygon, plan.obs_rows);
        printf("end\n");
    }
    return 0;
}
