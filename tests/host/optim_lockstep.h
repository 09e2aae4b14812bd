// Host shim (test infrastructure), beside lockstep.h: what csrc/irbpp_optim.hip uses beyond it.  __shfl_xor on a double (an
// exchange through a shared array between two barriers, like lockstep.h's), and float4 / make_float4 with the 16-byte
// alignment the device type has (the kernels take the float4 path only on addresses they tested for it).
#pragma once
#include "lockstep.h"

static double g_xd[LOCKSTEP_MAX_THREADS];
static inline double __shfl_xor(double v, int o) { return lockstep_shfl_xor(g_xd, v, o); }

struct alignas(16) float4 {
    float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
