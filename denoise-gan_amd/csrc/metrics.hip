// Image quality metrics: per-image error sums (PSNR) and SSIM of dense uint8 / fp32 NHWC images,
// accumulated in fp64 (include/dgan.h "Image quality metrics").  Every result is a fixed-order
// sum: integer atomics for the uint8 sums, block partials + one ordered pass for the rest.
#include "common.h"
#include <algorithm>
#include <cmath>

namespace dg {

constexpr int MT = 256;   // threads of every block in this file

// sum of v over the block (blockDim.x == MT), the same order on every run: a butterfly over each
// wave's lanes, then the four wave sums in wave order.  Valid in thread 0.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T *red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // (red may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---- error sums --------------------------------------------------------------------------------
constexpr int EB = 16;   // bytes per thread and load of the uint8 sums

__device__ __forceinline__ void u8_err_word(unsigned x, unsigned y, unsigned &sse, unsigned &sae) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((x >> (8 * k)) & 255u) - (int)((y >> (8 * k)) & 255u);
        sse += (unsigned)(d * d);
        sae += (unsigned)abs(d);
    }
}

// grid (blocks per image, n).  A thread's 32-bit sums hold 65025 * 16 per trip: it folds them into
// 64 bits every trip.
__global__ void __launch_bounds__(MT)
k_u8_err_sums(long count, const unsigned char *__restrict__ a, const unsigned char *__restrict__ b,
              unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long red[4];
    const unsigned char *pa = a + (long)blockIdx.y * count;
    const unsigned char *pb = b + (long)blockIdx.y * count;
    unsigned long long sse = 0, sae = 0;
    const long groups = (count + EB - 1) / EB;
    for (long g = (long)blockIdx.x * MT + threadIdx.x; g < groups; g += (long)gridDim.x * MT) {
        const long e = g * EB;
        unsigned s2 = 0, s1 = 0;
        if (e + EB <= count && ((((uintptr_t)(pa + e)) | ((uintptr_t)(pb + e))) & 15) == 0) {
            const uint4 x = *reinterpret_cast<const uint4 *>(pa + e);
            const uint4 y = *reinterpret_cast<const uint4 *>(pb + e);
            u8_err_word(x.x, y.x, s2, s1);
            u8_err_word(x.y, y.y, s2, s1);
            u8_err_word(x.z, y.z, s2, s1);
            u8_err_word(x.w, y.w, s2, s1);
        } else {
            const int m = (int)min((long)EB, count - e);
            for (int k = 0; k < m; ++k) {
                const int d = (int)pa[e + k] - (int)pb[e + k];
                s2 += (unsigned)(d * d);
                s1 += (unsigned)abs(d);
            }
        }
        sse += s2;
        sae += s1;
    }
    sse = block_sum(sse, red);
    sae = block_sum(sae, red);
    if (threadIdx.x == 0) {
        atomicAdd(&sums[2 * blockIdx.y], sse);
        atomicAdd(&sums[2 * blockIdx.y + 1], sae);
    }
}

// grid (P, n): partial[(image * P + block) * 2 + {0, 1}]
__global__ void __launch_bounds__(MT)
k_f32_err_partials(long count, const float *__restrict__ a, const float *__restrict__ b, double *__restrict__ partial) {
    __shared__ double red[4];
    const float *pa = a + (long)blockIdx.y * count;
    const float *pb = b + (long)blockIdx.y * count;
    double sse = 0.0, sae = 0.0;
    for (long e = (long)blockIdx.x * MT + threadIdx.x; e < count; e += (long)gridDim.x * MT) {
        const double d = (double)pa[e] - (double)pb[e];
        sse = fma(d, d, sse);
        sae += fabs(d);
    }
    sse = block_sum(sse, red);
    sae = block_sum(sae, red);
    if (threadIdx.x == 0) {
        double *p = partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = sse;
        p[1] = sae;
    }
}

// one block per image: out[image][q] = (its P partials [P][Q] summed -- thread t takes
// t, t + MT, ... in order, then the block sum) / div.  A division, not a product with 1 / div:
// count * (1.0 / count) is not 1.0 for many counts, count / count always is.
template <int Q>
__global__ void __launch_bounds__(MT)
k_sum_partials(int P, const double *__restrict__ partial, double div, double *__restrict__ out) {
    __shared__ double red[4];
    const double *p = partial + (long)blockIdx.x * P * Q;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        double s = 0.0;
        for (int i = threadIdx.x; i < P; i += MT) s += p[(long)i * Q + q];
        s = block_sum(s, red);
        if (threadIdx.x == 0) out[(long)blockIdx.x * Q + q] = s / div;
    }
}

static int err_blocks(long count) { return (int)std::max<long>(1, std::min<long>(dg_cdiv(count, (long)MT * 16), 1024)); }

// ---- SSIM --------------------------------------------------------------------------------------
constexpr int SW = 11;              // window taps
constexpr int STH = 16, STW = 32;   // map pixels per block tile
constexpr int SIH = STH + SW - 1;   // 26 input rows
constexpr int SIW = STW + SW - 1;   // 42 input columns
constexpr int SIS = SIW + 1;        // input row stride (words): odd, so the row pass's lanes (one
                                    // row each) read 26 different banks
constexpr int SHS = STW + 1;        // row-pass output row stride (doubles): lanes of different rows
                                    // write different bank pairs; the column pass reads along rows
constexpr int SHR = 4;              // row pass: outputs per thread (a run along the row)
constexpr int SVR = 2;              // column pass: outputs per thread (a run down the column)
static_assert(SIH * (STW / SHR) <= MT && STW * (STH / SVR) == MT, "one pass item per thread");

struct SsimArgs {
    int h, w, C;
    double scale, shift, c1, c2;
    double g[SW];
};

__device__ __forceinline__ float ssim_load(const unsigned char *p, long i) { return (float)p[i]; }
__device__ __forceinline__ float ssim_load(const float *p, long i) { return p[i]; }

// l * cs of one map pixel from its five moments; evaluated as written (no contraction), so two
// identical images give 1.0 exactly per pixel: num and den of both factors are then the same
// roundings (and the mean divides the exact sum of ones by their count)
__device__ __forceinline__ double ssim_pixel(double mua, double mub, double gaa, double gbb, double gab, double c1,
                                             double c2) {
#pragma clang fp contract(off)
    const double ab = mua * mub, aa = mua * mua, bb = mub * mub;
    const double l = (2.0 * ab + c1) / ((aa + bb) + c1);
    const double cs = (2.0 * (gab - ab) + c2) / (((gaa + gbb) - (aa + bb)) + c2);
    return l * cs;
}

// grid (tiles along w, tiles along h, n).  Per channel: the 26 x 42 input window of both images to
// LDS (raw values as fp32: exact for uint8 and fp32), the row pass over {a, b, a^2, b^2, ab} into
// fp64 LDS (26 rows x 32 columns x 5), the column pass and l * cs in registers.  One partial per
// block: partial[(image * gridDim.y + by) * gridDim.x + bx].
template <typename T>
__global__ void __launch_bounds__(MT)
k_ssim(SsimArgs A, const T *__restrict__ a, const T *__restrict__ b, double *__restrict__ partial) {
    __shared__ float in[2][SIH * SIS];
    __shared__ double hp[5][SIH * SHS];
    __shared__ double red[4];
    const int t = threadIdx.x;
    const int y0 = blockIdx.y * STH, x0 = blockIdx.x * STW;   // map = input origin of the tile
    const int mh = A.h - (SW - 1), mw = A.w - (SW - 1);
    const long img = (long)blockIdx.z * A.h * A.w * A.C;
    // row pass item: input row hr, outputs hx .. hx + SHR; column pass item: column vx, rows vy ..
    const int hr = t % SIH, hx = (t / SIH) * SHR;
    const int vx = t % STW, vy = (t / STW) * SVR;
    double acc = 0.0;
    for (int c = 0; c < A.C; ++c) {
        __syncthreads();   // the previous channel's passes are done with in / hp
        for (int e = t; e < SIH * SIW; e += MT) {
            const int r = e / SIW, q = e - r * SIW;
            const int y = y0 + r, x = x0 + q;
            float va = 0.f, vb = 0.f;
            if (y < A.h && x < A.w) {
                const long i = img + ((long)y * A.w + x) * A.C + c;
                va = ssim_load(a, i);
                vb = ssim_load(b, i);
            }
            in[0][r * SIS + q] = va;
            in[1][r * SIS + q] = vb;
        }
        __syncthreads();
        if (t < SIH * (STW / SHR)) {
            double s[5][SHR];
#pragma unroll
            for (int q = 0; q < 5; ++q)
#pragma unroll
                for (int o = 0; o < SHR; ++o) s[q][o] = 0.0;
#pragma unroll
            for (int k = 0; k < SHR + SW - 1; ++k) {
                const double va = fma((double)in[0][hr * SIS + hx + k], A.scale, A.shift);
                const double vb = fma((double)in[1][hr * SIS + hx + k], A.scale, A.shift);
                const double v[5] = {va, vb, va * va, vb * vb, va * vb};
#pragma unroll
                for (int o = 0; o < SHR; ++o) {
                    const int tap = k - o;
                    if (tap >= 0 && tap < SW) {
#pragma unroll
                        for (int q = 0; q < 5; ++q) s[q][o] = fma(A.g[tap], v[q], s[q][o]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 5; ++q)
#pragma unroll
                for (int o = 0; o < SHR; ++o) hp[q][hr * SHS + hx + o] = s[q][o];
        }
        __syncthreads();
        {
            double s[5][SVR];
#pragma unroll
            for (int q = 0; q < 5; ++q)
#pragma unroll
                for (int o = 0; o < SVR; ++o) s[q][o] = 0.0;
#pragma unroll
            for (int k = 0; k < SVR + SW - 1; ++k) {
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const double v = hp[q][(vy + k) * SHS + vx];
#pragma unroll
                    for (int o = 0; o < SVR; ++o) {
                        const int tap = k - o;
                        if (tap >= 0 && tap < SW) s[q][o] = fma(A.g[tap], v, s[q][o]);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < SVR; ++o)
                if (y0 + vy + o < mh && x0 + vx < mw)
                    acc += ssim_pixel(s[0][o], s[1][o], s[2][o], s[3][o], s[4][o], A.c1, A.c2);
        }
    }
    acc = block_sum(acc, red);
    if (t == 0) partial[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = acc;
}

struct SsimGrid {
    unsigned gx, gy;
    long tiles;
};
static SsimGrid ssim_grid(int h, int w) {
    SsimGrid g;
    g.gx = dg_cdiv(w - (SW - 1), STW);
    g.gy = dg_cdiv(h - (SW - 1), STH);
    g.tiles = (long)g.gx * g.gy;
    return g;
}
static bool ssim_shape_ok(int n, int h, int w, int C) {
    // (the grid's y and z limits; a partial count that k_sum_partials takes as an int)
    return n >= 0 && n <= 65535 && h >= SW && w >= SW && C >= 1 && h <= (1 << 20) && w <= (1 << 20) &&
           (long)h * w <= (1L << 34) && C <= 4096 && ssim_grid(h, w).gy <= 65535u && ssim_grid(h, w).tiles < (1L << 30);
}

template <typename T>
static int ssim_launch(const char *name, int n, int h, int w, int C, const T *a, const T *b, double scale, double shift,
                       double max_val, double *out, void *ws, size_t ws_bytes, hipStream_t stream) {
    DG_ARG(ssim_shape_ok(n, h, w, C), "bad shape: n %d h %d w %d C %d (SSIM needs h, w >= 11)", n, h, w, C);
    DG_ARG(max_val > 0.0 && std::isfinite(max_val) && std::isfinite(scale) && std::isfinite(shift),
           "max_val must be positive, scale and shift finite");
    if (n == 0) return DG_OK;
    DG_ARG(a && b && out, "NULL tensor");
    const SsimGrid g = ssim_grid(h, w);
    const size_t need = (size_t)n * g.tiles * sizeof(double);
    DG_ARG(ws && ws_bytes >= need && (((uintptr_t)ws) & 7) == 0, "workspace too small or misaligned: %zu < %zu bytes",
           ws_bytes, need);
    SsimArgs A;
    A.h = h; A.w = w; A.C = C;
    A.scale = scale; A.shift = shift;
    A.c1 = (0.01 * max_val) * (0.01 * max_val);
    A.c2 = (0.03 * max_val) * (0.03 * max_val);
    double sum = 0.0;
    for (int i = 0; i < SW; ++i) {
        A.g[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += A.g[i];
    }
    for (int i = 0; i < SW; ++i) A.g[i] /= sum;
    hipLaunchKernelGGL(k_ssim<T>, dim3(g.gx, g.gy, n), dim3(MT), 0, stream, A, a, b, (double *)ws);
    DG_LAUNCHED(name);
    const double count = (double)(h - (SW - 1)) * (double)(w - (SW - 1)) * (double)C;   // (exact: < 2^53)
    hipLaunchKernelGGL(k_sum_partials<1>, dim3(n), dim3(MT), 0, stream, (int)g.tiles, (const double *)ws, count, out);
    DG_LAUNCHED(name);
    return DG_OK;
}

}  // namespace dg

int dg_u8_err_sums(int n, int64_t count, const unsigned char *a, const unsigned char *b, uint64_t *sums,
                   dg_stream_t stream) {
    DG_ARG(n >= 0 && n <= 65535 && count >= 1 && count < (1LL << 46), "bad shape: n %d count %lld", n, (long long)count);
    if (n == 0) return DG_OK;
    DG_ARG(a && b && sums, "NULL tensor");
    DG_ARG((((uintptr_t)sums) & 7) == 0, "sums must be 8-byte aligned");
    const hipError_t e = hipMemsetAsync(sums, 0, (size_t)n * 2 * sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        dg::set_error("u8_err_sums: memset failed: %s", hipGetErrorString(e));
        return DG_ERR_HIP;
    }
    hipLaunchKernelGGL(dg::k_u8_err_sums, dim3(dg::err_blocks(count), n), dim3(dg::MT), 0, (hipStream_t)stream,
                       (long)count, a, b, reinterpret_cast<unsigned long long *>(sums));
    DG_LAUNCHED("u8_err_sums");
    return DG_OK;
}

int dg_err_sums_workspace_size(int n, int64_t count, size_t *bytes) {
    DG_ARG(bytes, "NULL output");
    DG_ARG(n >= 0 && n <= 65535 && count >= 1 && count < (1LL << 46), "bad shape: n %d count %lld", n, (long long)count);
    *bytes = (size_t)n * dg::err_blocks(count) * 2 * sizeof(double);
    return DG_OK;
}

int dg_f32_err_sums(int n, int64_t count, const float *a, const float *b, double *sums, void *ws, size_t ws_bytes,
                    dg_stream_t stream) {
    DG_ARG(n >= 0 && n <= 65535 && count >= 1 && count < (1LL << 46), "bad shape: n %d count %lld", n, (long long)count);
    if (n == 0) return DG_OK;
    DG_ARG(a && b && sums, "NULL tensor");
    const int P = dg::err_blocks(count);
    const size_t need = (size_t)n * P * 2 * sizeof(double);
    DG_ARG(ws && ws_bytes >= need && (((uintptr_t)ws) & 7) == 0, "workspace too small or misaligned: %zu < %zu bytes",
           ws_bytes, need);
    hipLaunchKernelGGL(dg::k_f32_err_partials, dim3(P, n), dim3(dg::MT), 0, (hipStream_t)stream, (long)count, a, b,
                       (double *)ws);
    DG_LAUNCHED("f32_err_sums");
    hipLaunchKernelGGL(dg::k_sum_partials<2>, dim3(n), dim3(dg::MT), 0, (hipStream_t)stream, P, (const double *)ws, 1.0,
                       sums);
    DG_LAUNCHED("f32_err_sums");
    return DG_OK;
}

int dg_ssim_workspace_size(int n, int h, int w, int C, size_t *bytes) {
    DG_ARG(bytes, "NULL output");
    DG_ARG(dg::ssim_shape_ok(n, h, w, C), "bad shape: n %d h %d w %d C %d (SSIM needs h, w >= 11)", n, h, w, C);
    *bytes = (size_t)n * dg::ssim_grid(h, w).tiles * sizeof(double);
    return DG_OK;
}

int dg_ssim_u8(int n, int h, int w, int C, const unsigned char *a, const unsigned char *b, double max_val, double *out,
               void *ws, size_t ws_bytes, dg_stream_t stream) {
    return dg::ssim_launch("ssim_u8", n, h, w, C, a, b, 1.0, 0.0, max_val, out, ws, ws_bytes, (hipStream_t)stream);
}

int dg_ssim_f32(int n, int h, int w, int C, const float *a, const float *b, double scale, double shift, double max_val,
                double *out, void *ws, size_t ws_bytes, dg_stream_t stream) {
    return dg::ssim_launch("ssim_f32", n, h, w, C, a, b, scale, shift, max_val, out, ws, ws_bytes, (hipStream_t)stream);
}
