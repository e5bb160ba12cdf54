// BM3D, stage 1, on dense uint8 RGB frames (include/dgan.h "BM3D"; the integer definition and its
// numpy reference: dgan/filters.py bm3d_ref).  Block matching, hard thresholding of each group's
// 3-D Walsh-Hadamard transform, aggregation.  Integers only; the only order-dependent step is the
// aggregation, whose uint32 atomic adds commute: two calls give the same bits.
//
//   k_bm3d_clear   zeroes the num / den planes (a kernel, so that a call can be captured)
//   k_bm3d         a workgroup of 256 threads (4 waves) owns a tile of 8 x 8 reference patches: with
//                  the step of 3 they cover 29 x 29 pixels.  These and the rs = search / 2 pixels
//                  around them that the candidates reach, 29 + 2 rs a side, are staged once into
//                  LDS, a pixel per dword (bytes R G B 0, reflection resolved here).
//     matching     D = N(ref) + N(cand) - 2 C: N, the 8 x 8 box sums of the pixels' own squares, is
//                  formed once per tile, separably (row sums, then column sums).  The cross term C
//                  of one offset d is an 8 x 8 box sum of c_d(u) = dot4(P(u), P(u + d)) sampled at
//                  the reference corners; neighbouring references share 5 of their 8 rows and
//                  columns, so it is formed separably too:
//                    phase 1  232 threads = 8 reference rows x 29 columns: the 8 products of one
//                             column of one reference row (one v_dot4_u32_u8 each, the base pixels
//                             in registers for every offset), summed: V
//                    barrier
//                    phase 2  64 threads, one per reference: 8 values of V, D, and the sort key
//                             (D << 9) | idx (D <= 480000 < 2^19, idx < 441), or all ones for a
//                             candidate that does not match; the key goes to LDS
//                  V is double-buffered: one barrier per offset (as k_nlm's H).  29 dot products
//                  per reference and offset in place of 64.
//     selection    the keys of 7 rows of offsets (at most 147 per reference) fill the key buffer;
//                  then every wave takes 16 references in turn: a lane holds up to 3 keys and one
//                  of the 15 best so far, and K - 1 rounds each take the wave-wide minimum (six
//                  xor steps) and retire it from the lane that held it (keys are distinct: idx
//                  is).  No lane walks the candidates, and no key leaves LDS.
//     filter       a wave per group, a lane per pixel of the 8 x 8 patch, the m x 3 values of its
//                  pixel in registers (m = 1, 2, 4, 8, 16: one instantiation each, every index
//                  static).  Along the group: in-register butterflies.  Across the patch: six
//                  xor-butterfly stages over the lane index, which IS H8 (x) H8 in Sylvester order
//                  (xor 1, 2: DPP quad permutes; 4, 8, 16: ds_swizzle; 32: ds_bpermute).  The kept
//                  count N comes from ballots and popcounts; the inverse is the same code.
//     aggregation  w E and w are added with uint32 atomics: in LDS for the centre of the staged
//                  area (as much of it as fits in the key buffer, which is free by then: all of it
//                  up to search 11, 42 x 42 of 49 x 49 at search 21), in the global planes for
//                  the rest; the LDS part is flushed with one atomic per touched value.  Only
//                  pixels inside the image are touched.
//   k_bm3d_divide  out = (num + 2 den) / (4 den)
//
// LDS at search 21: pixels 49 x 49, N 42 x 42, V 2 x 8 x 29, best 64 x 16, counts 64, and the shared
// buffer (keys 64 x 147 | row sums 49 x 42 | accumulators 42 x 42 x 6) 10584 dwords: 65204 bytes.
#include "bm3d_common.h"

namespace dg {

// One group: reference (ry, rx) of the tile with the M - 1 first entries of its best list.
template <int M>
__device__ __forceinline__ void filter_group(const Bm3dGeom &g, const int *P, const unsigned *best, unsigned *acc,
                                             unsigned *num, unsigned *den, int y_org, int x_org, int ry, int rx,
                                             int lane) {
    constexpr int LOG = M == 1 ? 0 : M == 2 ? 1 : M == 4 ? 2 : M == 8 ? 3 : 4;
    const int py = lane >> 3, px = lane & 7, T = g.T[LOG];
    int ly[M], lx[M];
    unsigned q[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        int dy = 0, dx = 0;
        if (k) {
            const int idx = (int)(best[k - 1] & 511u);
            dy = idx / g.s - g.rs;
            dx = idx - (dy + g.rs) * g.s - g.rs;
        }
        ly[k] = BSTEP * ry + g.rs + dy + py;
        lx[k] = BSTEP * rx + g.rs + dx + px;
        q[k] = (unsigned)P[ly[k] * g.se + lx[k]];
    }
    unsigned we[M][3], wgt[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int x[M];
#pragma unroll
        for (int k = 0; k < M; ++k) x[k] = (int)((q[k] >> (8 * c)) & 255u);
        group_wht<M>(x);
        int kept = 0;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            x[k] = patch_wht(x[k], lane);
            const bool keep = abs(x[k]) > T || (k == 0 && lane == 0);
            kept += __popcll(__ballot(keep));
            x[k] = keep ? x[k] : 0;
        }
        group_wht<M>(x);
        wgt[c] = (unsigned)max(1, 1024 / max(kept, 1));
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const int v = patch_wht(x[k], lane);
            we[k][c] = wgt[c] * (unsigned)min(max((v + 8 * M) >> (4 + LOG), 0), 1020);
        }
    }
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const int gy = y_org + ly[k], gx = x_org + lx[k];
        if (gy < 0 || gy >= g.h || gx < 0 || gx >= g.w) continue;
        const int ay = ly[k] - g.a0, ax = lx[k] - g.a0;
        if (ay >= 0 && ay < g.ae && ax >= 0 && ax < g.ae) {
            unsigned *a = acc + (ay * g.ae + ax) * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicAdd(a + c, we[k][c]);
                atomicAdd(a + 3 + c, wgt[c]);
            }
        } else {
            const long o = ((long)gy * g.w + gx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicAdd(num + o + c, we[k][c]);
                atomicAdd(den + o + c, wgt[c]);
            }
        }
    }
}

// grid (tiles along the reference columns, tiles along the reference rows, n); dynamic LDS
__global__ void __launch_bounds__(BT)
k_bm3d(Bm3dGeom g, const unsigned char *__restrict__ in, unsigned *__restrict__ num, unsigned *__restrict__ den) {
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
    in += image;
    num += image;
    den += image;

    // the tile and its apron, reflected into the image; empty best lists
    for (int i = tid; i < se * se; i += BT) {
        const int ly = i / se, lx = i - ly * se;
        const unsigned char *p = in + ((long)breflect(y_org + ly, g.h) * g.w + breflect(x_org + lx, g.w)) * 3;
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
                    if (D <= BMATCH) key = (D << 9) | (unsigned)((dy + rs) * s + dx + rs);
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
        if (members >= 16) filter_group<16>(g, P, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else if (members >= 8) filter_group<8>(g, P, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else if (members >= 4) filter_group<4>(g, P, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else if (members >= 2) filter_group<2>(g, P, b, acc, num, den, y_org, x_org, ry, rx, lane);
        else filter_group<1>(g, P, b, acc, num, den, y_org, x_org, ry, rx, lane);
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

__global__ void __launch_bounds__(256) k_bm3d_clear(long count, unsigned *__restrict__ sums) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) sums[i] = 0u;
}

__global__ void __launch_bounds__(256)
k_bm3d_divide(long count, const unsigned *__restrict__ num, const unsigned *__restrict__ den,
              unsigned char *__restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
        const unsigned d = max(den[i], 1u);   // (den >= 1: every pixel lies in a reference patch)
        out[i] = (unsigned char)((num[i] + 2u * d) / (4u * d));
    }
}

static int isqrt_int(long v) {
    long r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (int)r;
}

}  // namespace dg

int dg_bm3d_ws_bytes(int n, int h, int w, size_t *ws_bytes) {
    DG_ARG(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= (1 << 16) && w <= (1 << 16) && ws_bytes,
           "bm3d_ws_bytes: bad shape: n %d, %dx%d", n, h, w);
    *ws_bytes = (size_t)n * h * w * 3 * 2 * sizeof(unsigned);
    return DG_OK;
}

namespace dg {

int bm3d_prepare(const char *name, int n, int h, int w, int sigma, int search, int group, const void *in, const void *ws,
                 size_t ws_bytes, const void *out, Bm3dGeom *geom, size_t *lds_bytes) {
    size_t need = 0;
    if (int rc = dg_bm3d_ws_bytes(n, h, w, &need)) return rc;
    DG_ARG(sigma >= 1 && sigma <= 40, "%s: sigma must be in 1..40, got %d", name, sigma);
    DG_ARG(search >= 3 && search <= 2 * BRS + 1 && (search & 1), "%s: the search window must be odd in 3..%d, got %d",
           name, 2 * BRS + 1, search);
    DG_ARG(group == 2 || group == 4 || group == 8 || group == 16, "%s: the group must be 2, 4, 8 or 16, got %d", name,
           group);
    if (n == 0) return DG_OK;
    DG_ARG(in && out && ws, "%s: NULL tensor", name);
    DG_ARG(in != out, "%s: the output must not be the input", name);
    DG_ARG(ws_bytes >= need, "%s: the workspace holds %zu bytes, %zu needed", name, ws_bytes, need);
    Bm3dGeom &g = *geom;
    g.h = h;
    g.w = w;
    g.nry = (h + BP - 2) / BSTEP + 1;   // corners -7 + 3 a <= h - 1
    g.nrx = (w + BP - 2) / BSTEP + 1;
    g.s = search;
    g.rs = search / 2;
    g.K = group;
    g.se = BEXT + 2 * g.rs;
    g.ne = BEXT - BP + 1 + 2 * g.rs;
    const int fixed = g.se * g.se + g.ne * g.ne + 2 * BR * BEXT + BR * BR * BBEST + BR * BR;
    const int room = BLDS_MAX / 4 - fixed;
    g.ae = isqrt_int(room / 6);
    if (g.ae > g.se) g.ae = g.se;
    g.a0 = (g.se - g.ae) / 2;
    g.shared = BR * BR * (search < BROWS ? search : BROWS) * search;
    if (g.shared < g.se * g.ne) g.shared = g.se * g.ne;
    if (g.shared < g.ae * g.ae * 6) g.shared = g.ae * g.ae * 6;
    for (int l = 0; l < 5; ++l) g.T[l] = isqrt_int(729L * sigma * sigma * BP * BP * (1 << l) / 100);
    *lds_bytes = (size_t)(fixed + g.shared) * sizeof(int);
    DG_ARG(*lds_bytes <= (size_t)BLDS_MAX, "%s: %zu bytes of LDS", name, *lds_bytes);
    return DG_OK;
}

static unsigned sweep_blocks(long count) { return (unsigned)((count + 255) / 256 < 65536 ? (count + 255) / 256 : 65536); }

void bm3d_clear(long count, unsigned *sums, dg_stream_t stream) {
    hipLaunchKernelGGL(k_bm3d_clear, dim3(sweep_blocks(count)), dim3(256), 0, (hipStream_t)stream, count, sums);
}

void bm3d_divide(long count, const unsigned *num, const unsigned *den, unsigned char *out, dg_stream_t stream) {
    hipLaunchKernelGGL(k_bm3d_divide, dim3(sweep_blocks(2 * count)), dim3(256), 0, (hipStream_t)stream, count, num, den,
                       out);
}

}  // namespace dg

int dg_bm3d_u8(int n, int h, int w, int sigma, int search, int group, const unsigned char *in, void *ws,
               size_t ws_bytes, unsigned char *out, dg_stream_t stream) {
    using namespace dg;
    const char *name = "bm3d_u8";
    Bm3dGeom g;
    size_t lds = 0;
    if (int rc = bm3d_prepare(name, n, h, w, sigma, search, group, in, ws, ws_bytes, out, &g, &lds)) return rc;
    if (n == 0) return DG_OK;
    const long count = (long)n * h * w * 3;
    unsigned *num = static_cast<unsigned *>(ws), *den = num + count;
    bm3d_clear(2 * count, num, stream);
    hipLaunchKernelGGL(k_bm3d, dim3(dg_cdiv(g.nrx, BR), dg_cdiv(g.nry, BR), n), dim3(BT), lds, (hipStream_t)stream, g, in,
                       num, den);
    bm3d_divide(count, num, den, out, stream);
    DG_LAUNCHED(name);
    return DG_OK;
}
