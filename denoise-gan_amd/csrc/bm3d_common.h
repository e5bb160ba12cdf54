// What the two BM3D stages (bm3d.hip, bm3d_wiener.hip) share: the tile's constants and geometry, the
// lane butterflies of the Walsh-Hadamard transform, and the host steps around the tile kernel.
#pragma once
#include "common.h"

namespace dg {

constexpr int BT = 256;                       // threads of a workgroup
constexpr int BR = 8;                         // reference patches per tile side
constexpr int BP = 8, BSTEP = 3;              // patch side, reference step
constexpr int BEXT = BSTEP * (BR - 1) + BP;   // pixels a tile's reference patches cover: 29
constexpr int BRS = 10;                       // largest search radius
constexpr int BROWS = 7;                      // rows of offsets per selection
constexpr int BBEST = 16;                     // dwords per reference's best list (15 used)
constexpr unsigned BNONE = 0xffffffffu;       // the key of a candidate that does not match
constexpr unsigned BMATCH = 480000u;
constexpr int BLDS_MAX = 64 * 1024;
static_assert(BR * BEXT <= BT && BR * BR <= BT, "phase 1 / phase 2: one thread per role");

struct Bm3dGeom {
    int h, w, nry, nrx;   // image, reference grid
    int s, rs, K;         // search, its radius, group size
    int se, ne;           // staged extent 29 + 2 rs, extent of N 22 + 2 rs
    int ae, a0;           // accumulator extent in LDS and its first staged row / column
    int shared;           // dwords of the shared buffer
    int T[5];             // thresholds of m = 1, 2, 4, 8, 16
};

// np.pad's "reflect" for any pad width (dgan/infer.py pad_index)
__device__ __forceinline__ int breflect(int v, int size) {
    if (size == 1) return 0;
    const int p = 2 * (size - 1);
    int j = v % p;
    if (j < 0) j += p;
    return j >= size ? p - j : j;
}

// the value of lane ^ MASK
template <int MASK>
__device__ __forceinline__ int lane_xor(int v) {
    if constexpr (MASK == 1) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);        // quad_perm [1,0,3,2]
    else if constexpr (MASK == 2) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    else if constexpr (MASK < 32) return __builtin_amdgcn_ds_swizzle(v, (MASK << 10) | 0x1f);  // and 31, or 0, xor MASK
    else return __shfl_xor(v, 32);
}

template <int MASK>
__device__ __forceinline__ int lane_butterfly(int v, int lane) {
    const int o = lane_xor<MASK>(v);
    return (lane & MASK) ? o - v : v + o;
}

// H8 (x) H8 over the 64 lanes (lane = 8 row + column), unnormalised
__device__ __forceinline__ int patch_wht(int v, int lane) {
    v = lane_butterfly<1>(v, lane);
    v = lane_butterfly<2>(v, lane);
    v = lane_butterfly<4>(v, lane);
    v = lane_butterfly<8>(v, lane);
    v = lane_butterfly<16>(v, lane);
    return lane_butterfly<32>(v, lane);
}

// H_M along the group, Sylvester order, in registers
template <int M>
__device__ __forceinline__ void group_wht(int (&x)[M]) {
#pragma unroll
    for (int len = 1; len < M; len <<= 1)
#pragma unroll
        for (int i = 0; i < M; i += 2 * len)
#pragma unroll
            for (int j = i; j < i + len; ++j) {
                const int a = x[j], b = x[j + len];
                x[j] = a + b;
                x[j + len] = a - b;
            }
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}

// host side (bm3d.hip): argument checks and the tile geometry; the clear and divide launches
int bm3d_prepare(const char *name, int n, int h, int w, int sigma, int search, int group, const void *in, const void *ws,
                 size_t ws_bytes, const void *out, Bm3dGeom *g, size_t *lds);
void bm3d_clear(long count, unsigned *sums, dg_stream_t stream);
void bm3d_divide(long count, const unsigned *num, const unsigned *den, unsigned char *out, dg_stream_t stream);

}  // namespace dg
