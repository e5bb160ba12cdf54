// BM3D, stage 2, on dense uint8 RGB frames (include/dgan.h "BM3D"; the integer definition and its
// numpy reference: dgan/filters.py bm3d_wiener_ref).  Block matching on a pilot estimate, a Wiener
// weight per coefficient of the group's 3-D Walsh-Hadamard transform, aggregation.  Integers only
// (one fp32 reciprocal seeds an integer division whose result is corrected to the exact quotient).
//
//   k_bm3d_wiener  the tile, its LDS plan and its three phases are stage 1's (bm3d.hip), kept as a
//                  copy of its own so that stage 1's code object does not move.  What differs:
//     matching     the PILOT is staged and matched, at D <= 76800.  The noisy frame is not staged:
//                  at search 21 stage 1's plan already fills 65204 of the 65536 bytes.
//     filter       a wave per group, a lane per pixel of the 8 x 8 patch.  The pilot's m pixels come
//                  from LDS, the noisy ones from global memory (m reflected 3-byte gathers a lane;
//                  the 64 lanes of a member read 8 runs of 24 bytes).  One channel at a time: both
//                  groups' m values in registers, the forward transform of each, then per
//                  coefficient
//                    e  = min(Cy^2 >> (6 + log2 m), 2^23)       v_mul_lo / v_mul_hi
//                    Wq = (256 e + d / 2) / d,  d = e + sigma^2  (wiener_weight)
//                    F  = (Wq Cz + 128) >> 8
//                  F overwrites the noisy registers, the pilot's are dead from here; the inverse
//                  transform runs on F.  Sum Wq^2 is a lane sum and six xor steps over the wave.
//     aggregation  channel by channel straight from the registers (no m x 3 products are kept), the
//                  member's position packed in one register.
#include "bm3d_common.h"

namespace dg {

constexpr unsigned BMATCH2 = 76800u;          // 400 per sample * 192 samples
constexpr unsigned BENERGY_MAX = 1u << 23;    // from here on Wq = 256 for every sigma <= 40

// (256 e + d / 2) / d with d = e + sigma2, exactly; e <= 2^23, 1 <= sigma2 <= 1600.
// d < 2^24 is exact in fp32; n = 256 e + d / 2 < 2^32 rounds by at most 2^-24 of itself, v_rcp_f32 is
// good to 1 ulp and the product rounds once more: the estimate is off by less than 2^-22 of a quotient
// that is at most 256.5, far below 1, so its floor is the quotient or a neighbour of it, and one step
// either way lands on it.  q d <= 257 (2^23 + 1600) < 2^32.
__device__ __forceinline__ unsigned wiener_weight(unsigned e, unsigned sigma2) {
    const unsigned d = e + sigma2, n = (e << 8) + (d >> 1);
    unsigned q = (unsigned)((float)n * __builtin_amdgcn_rcpf((float)d));
    const unsigned p = q * d;
    if (p > n) --q;
    else if (n - p >= d) ++q;
    return q;
}

__device__ __forceinline__ unsigned wave_sum(unsigned u) {
    int v = (int)u;
    v += lane_xor<1>(v);
    v += lane_xor<2>(v);
    v += lane_xor<4>(v);
    v += lane_xor<8>(v);
    v += lane_xor<16>(v);
    v += lane_xor<32>(v);
    return (unsigned)v;
}

// One group: reference (ry, rx) of the tile with the M - 1 first entries of its best list.
template <int M>
__device__ __forceinline__ void wiener_group(const Bm3dGeom &g, unsigned sigma2, const int *P,
                                             const unsigned char *__restrict__ noisy, const unsigned *best,
                                             unsigned *acc, unsigned *num, unsigned *den, int y_org, int x_org, int ry,
                                             int rx, int lane) {
    constexpr int LOG = M == 1 ? 0 : M == 2 ? 1 : M == 4 ? 2 : M == 8 ? 3 : 4;
    const int py = lane >> 3, px = lane & 7;
    int pos[M];              // staged row | staged column << 8 (both < 49)
    unsigned qy[M], qz[M];   // the member's pilot and noisy pixel, bytes R G B 0
#pragma unroll
    for (int k = 0; k < M; ++k) {
        int dy = 0, dx = 0;
        if (k) {
            const int idx = (int)(best[k - 1] & 511u);
            dy = idx / g.s - g.rs;
            dx = idx - (dy + g.rs) * g.s - g.rs;
        }
        const int ly = BSTEP * ry + g.rs + dy + py, lx = BSTEP * rx + g.rs + dx + px;
        pos[k] = ly | (lx << 8);
        qy[k] = (unsigned)P[ly * g.se + lx];
        const unsigned char *p = noisy + ((long)breflect(y_org + ly, g.h) * g.w + breflect(x_org + lx, g.w)) * 3;
        qz[k] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    }
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        int y[M], z[M];
#pragma unroll
        for (int k = 0; k < M; ++k) {
            y[k] = (int)((qy[k] >> (8 * c)) & 255u);
            z[k] = (int)((qz[k] >> (8 * c)) & 255u);
        }
        group_wht<M>(y);
        group_wht<M>(z);
        unsigned sq = 0;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const int cy = patch_wht(y[k], lane), cz = patch_wht(z[k], lane);
            const unsigned a = (unsigned)abs(cy);                                        // < 2^18
            const unsigned long long e64 = ((unsigned long long)a * a) >> (6 + LOG);     // < 2^26
            const unsigned e = (unsigned)min(e64, (unsigned long long)BENERGY_MAX);
            const unsigned wq = (k == 0 && lane == 0) ? 256u : wiener_weight(e, sigma2);   // DC stays
            sq += wq * wq;
            z[k] = ((int)wq * cz + 128) >> 8;
        }
        group_wht<M>(z);
        const unsigned n2 = max(1u, (wave_sum(sq) + (1u << 15)) >> 16);
        const unsigned wgt = max(1u, 1024u / n2);
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const int v = patch_wht(z[k], lane);
            const unsigned we = wgt * (unsigned)min(max((v + 8 * M) >> (4 + LOG), 0), 1020);
            const int ly = pos[k] & 255, lx = pos[k] >> 8;
            const int gy = y_org + ly, gx = x_org + lx;
            if (gy < 0 || gy >= g.h || gx < 0 || gx >= g.w) continue;
            const int ay = ly - g.a0, ax = lx - g.a0;
            if (ay >= 0 && ay < g.ae && ax >= 0 && ax < g.ae) {
                unsigned *a = acc + (ay * g.ae + ax) * 6 + c;
                atomicAdd(a, we);
                atomicAdd(a + 3, wgt);
            } else {
                const long o = ((long)gy * g.w + gx) * 3 + c;
                atomicAdd(num + o, we);
                atomicAdd(den + o, wgt);
            }
        }
    }
}

// grid (tiles along the reference columns, tiles along the reference rows, n); dynamic LDS
__global__ void __launch_bounds__(BT)
k_bm3d_wiener(Bm3dGeom g, unsigned sigma2, const unsigned char *__restrict__ noisy,
              const unsigned char *__restrict__ pilot, unsigned *__restrict__ num, unsigned *__restrict__ den) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    const int se = g.se, ne = g.ne, rs = g.rs, s = g.s;
    int *P = lds, *Nb = P + se * se, *V = Nb + ne * ne;
    unsigned *best = reinterpret_cast<unsigned *>(V + 2 * BR * BEXT);
    int *taken = reinterpret_cast<int *>(best + BR * BR * BBEST);
    unsigned *keys = reinterpret_cast<unsigned *>(taken + BR * BR);   // the shared buffer
    const int kstride = min(BROWS, s) * s;                            // key slots of a reference
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y_org = 1 - BP + BSTEP * BR * (int)blockIdx.y - rs, x_org = 1 - BP + BSTEP * BR * (int)blockIdx.x - rs;
    const long image = (long)blockIdx.z * g.h * g.w * 3;
    noisy += image;
    pilot += image;
    num += image;
    den += image;

    // the pilot's tile and its apron, reflected into the image; empty best lists
    for (int i = tid; i < se * se; i += BT) {
        const int ly = i / se, lx = i - ly * se;
        const unsigned char *p = pilot + ((long)breflect(y_org + ly, g.h) * g.w + breflect(x_org + lx, g.w)) * 3;
        P[i] = (int)((unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16));
    }
    for (int i = tid; i < BR * BR * BBEST; i += BT) best[i] = BNONE;
    __syncthreads();
    // N[u][v] = the 8 x 8 box sum of the pixels' own squares from staged (u, v) on: rows, then columns
    int *rowsum = reinterpret_cast<int *>(keys);
    for (int i = tid; i < se * ne; i += BT) {
        const int u = i / ne, v = i - u * ne;
        unsigned sum = 0;
#pragma unroll
        for (int k = 0; k < BP; ++k) {
            const unsigned q = (unsigned)P[u * se + v + k];
            sum = __builtin_amdgcn_udot4(q, q, sum, false);
        }
        rowsum[i] = (int)sum;
    }
    __syncthreads();
    for (int i = tid; i < ne * ne; i += BT) {
        const int u = i / ne, v = i - u * ne;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < BP; ++k) sum += rowsum[(u + k) * ne + v];
        Nb[i] = sum;
    }
    __syncthreads();

    // phase 1 role: reference row r1, extent column c1; its 8 base pixels stay in registers
    const bool p1 = tid < BR * BEXT;
    const int r1 = p1 ? tid / BEXT : 0, c1 = p1 ? tid - r1 * BEXT : 0;
    const int *pa = P + (BSTEP * r1 + rs) * se + c1 + rs;
    unsigned a[BP];
#pragma unroll
    for (int k = 0; k < BP; ++k) a[k] = (unsigned)pa[k * se];
    // phase 2 role: reference (r2, c2) of the tile
    const int r2 = (tid >> 3) & (BR - 1), c2 = tid & (BR - 1);
    const bool p2 = tid < BR * BR && BR * (int)blockIdx.y + r2 < g.nry && BR * (int)blockIdx.x + c2 < g.nrx;
    const int *pn = Nb + (BSTEP * r2 + rs) * ne + BSTEP * c2 + rs;
    const int Nref = pn[0];

    int buf = 0;
    for (int row0 = 0; row0 < s; row0 += BROWS) {
        const int rows = min(BROWS, s - row0), count = rows * s;
        for (int j = 0; j < count; ++j) {
            const int jy = j / s, dy = row0 + jy - rs, dx = j - jy * s - rs;
            int *Vb = V + buf * BR * BEXT;
            if (p1) {
                const int *pb = pa + dy * se + dx;
                unsigned sum = 0;
#pragma unroll
                for (int k = 0; k < BP; ++k) sum = __builtin_amdgcn_udot4(a[k], (unsigned)pb[k * se], sum, false);
                Vb[tid] = (int)sum;
            }
            __syncthreads();   // the one barrier of an offset: V written -> V read
            if (tid < BR * BR) {
                unsigned key = BNONE;
                if (p2 && (dy | dx)) {
                    const int *pv = Vb + r2 * BEXT + BSTEP * c2;
                    int cross = 0;
#pragma unroll
                    for (int k = 0; k < BP; ++k) cross += pv[k];
                    const unsigned D = (unsigned)(Nref + pn[dy * ne + dx] - 2 * cross);
                    if (D <= BMATCH2) key = (D << 9) | (unsigned)((dy + rs) * s + dx + rs);
                }
                keys[tid * kstride + j] = key;
            }
            buf ^= 1;
        }
        __syncthreads();   // keys written -> keys read
        // selection: the K - 1 smallest of a reference's keys and its best so far
        for (int r = wave * (BR * BR / 4); r < (wave + 1) * (BR * BR / 4); ++r) {
            const unsigned *kr = keys + r * kstride;
            unsigned k0 = lane < count ? kr[lane] : BNONE;
            unsigned k1 = lane + 64 < count ? kr[lane + 64] : BNONE;
            unsigned k2 = lane + 128 < count ? kr[lane + 128] : BNONE;
            unsigned kb = lane < BBEST ? best[r * BBEST + lane] : BNONE;
            int got = 0;
            for (; got < g.K - 1; ++got) {
                const unsigned m = wave_min(min(min(k0, k1), min(k2, kb)));
                if (m == BNONE) break;
                if (lane == 0) best[r * BBEST + got] = m;
                k0 = k0 == m ? BNONE : k0;
                k1 = k1 == m ? BNONE : k1;
                k2 = k2 == m ? BNONE : k2;
                kb = kb == m ? BNONE : kb;
            }
            if (lane >= got && lane < BBEST) best[r * BBEST + lane] = BNONE;
            if (lane == 0) taken[r] = got;
        }
        __syncthreads();   // keys read -> the next rows' keys (or the accumulators) written
    }

    // the accumulators take the shared buffer
    unsigned *acc = keys;
    for (int i = tid; i < g.ae * g.ae * 6; i += BT) acc[i] = 0u;
    __syncthreads();

    // collaborative filtering: a wave per group
    for (int r = wave * (BR * BR / 4); r < (wave + 1) * (BR * BR / 4); ++r) {
        const int ry = r >> 3, rx = r & (BR - 1);
        if (BR * (int)blockIdx.y + ry >= g.nry || BR * (int)blockIdx.x + rx >= g.nrx) continue;
        const int members = 1 + __builtin_amdgcn_readfirstlane(taken[r]);
        const unsigned *b = best + r * BBEST;
        if (members >= 16) wiener_group<16>(g, sigma2, P, noisy, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else if (members >= 8) wiener_group<8>(g, sigma2, P, noisy, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else if (members >= 4) wiener_group<4>(g, sigma2, P, noisy, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else if (members >= 2) wiener_group<2>(g, sigma2, P, noisy, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else wiener_group<1>(g, sigma2, P, noisy, b, acc, num, den, y_org, x_org, ry, rx, lane);
    }
    __syncthreads();

    // the touched accumulators go to the global planes
    for (int i = tid; i < g.ae * g.ae * 3; i += BT) {
        const int pix = i / 3, c = i - pix * 3;
        const unsigned d = acc[pix * 6 + 3 + c];
        if (!d) continue;
        const int ay = pix / g.ae, gy = y_org + g.a0 + ay, gx = x_org + g.a0 + pix - ay * g.ae;
        if (gy < 0 || gy >= g.h || gx < 0 || gx >= g.w) continue;
        const long o = ((long)gy * g.w + gx) * 3 + c;
        atomicAdd(num + o, acc[pix * 6 + c]);
        atomicAdd(den + o, d);
    }
}

}  // namespace dg

int dg_bm3d_wiener_u8(int n, int h, int w, int sigma, int search, int group, const unsigned char *in,
                      const unsigned char *pilot, void *ws, size_t ws_bytes, unsigned char *out, dg_stream_t stream) {
    using namespace dg;
    const char *name = "bm3d_wiener_u8";
    Bm3dGeom g;
    size_t lds = 0;
    if (int rc = bm3d_prepare(name, n, h, w, sigma, search, group, in, ws, ws_bytes, out, &g, &lds)) return rc;
    if (n == 0) return DG_OK;
    DG_ARG(pilot, "%s: NULL tensor", name);
    DG_ARG(pilot != out, "%s: the output must not be the pilot", name);
    const long count = (long)n * h * w * 3;
    unsigned *num = static_cast<unsigned *>(ws), *den = num + count;
    bm3d_clear(2 * count, num, stream);
    hipLaunchKernelGGL(k_bm3d_wiener, dim3(dg_cdiv(g.nrx, BR), dg_cdiv(g.nry, BR), n), dim3(BT), lds, (hipStream_t)stream,
                       g, (unsigned)(sigma * sigma), in, pilot, num, den);
    bm3d_divide(count, num, den, out, stream);
    DG_LAUNCHED(name);
    return DG_OK;
}
