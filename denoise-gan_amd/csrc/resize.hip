// Image resize by 4-tap tables (include/dgan.h "Image resize"; the tables and the fp64 reference
// with the same evaluation order: dgan/resize.py).  One launch, no intermediate in HBM: a block owns
// an output tile of one image, runs the vertical pass from global memory into an fp64 LDS strip
// over the tile's window of input columns, then the horizontal pass as a 4-tap gather from LDS.
#include "common.h"
#include <cmath>

namespace dg {

constexpr int RT = 256;            // threads per block
constexpr int RTH = 8, RTW = 64;   // output pixels per block tile
constexpr int RCAP = 6400;         // doubles of the strip (50 KB): x4 down at C 3 is a window of
                                   // (4 * 64 + 3) * 3 = 777 elements, 8 rows of it 6216
static_assert(RTW * 4 == RT, "one column tap per thread at the table load");

struct ResizeArgs {
    int hi, wi, C, ho, wo;
    double mul, bias;
};

// the tile's slice of the tables, indices clamped into the image
struct ResizeTile {
    double wy[RTH * 4], wx[RTW * 4];
    int iy[RTH * 4], ix[RTW * 4];
};

// ((w0 a0 + w1 a1) + w2 a2) + w3 a3, every product and sum rounded on its own
__host__ __device__ __forceinline__ double resize_tap4(const double *w, double a0, double a1, double a2, double a3) {
#pragma clang fp contract(off)
    return ((w[0] * a0 + w[1] * a1) + w[2] * a2) + w[3] * a3;
}

// m <= 4 consecutive elements as doubles: one wide load where p is aligned, else one by one
__host__ __device__ __forceinline__ void resize_load4(const unsigned char *p, int m, double v[4]) {
    if (m == 4 && (((uintptr_t)p) & 3) == 0) {
        const unsigned x = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (double)((x >> (8 * j)) & 255u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < m ? (double)p[j] : 0.0;
    }
}
__host__ __device__ __forceinline__ void resize_load4(const float *p, int m, double v[4]) {
    if (m == 4 && (((uintptr_t)p) & 15) == 0) {
        const float4 x = *reinterpret_cast<const float4 *>(p);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < m ? (double)p[j] : 0.0;
    }
}

__host__ __device__ __forceinline__ unsigned char resize_cvt(double v, const ResizeArgs &A, unsigned char) {
#pragma clang fp contract(off)
    const double x = v * A.mul + A.bias;
    return (unsigned char)floor(fmin(fmax(x, 0.0), 255.0));
}
__host__ __device__ __forceinline__ float resize_cvt(double v, const ResizeArgs &, float) { return (float)v; }

__host__ __device__ __forceinline__ void resize_store4(unsigned char *p, int m, const unsigned char v[4]) {
    if (m == 4 && (((uintptr_t)p) & 3) == 0) {
        *reinterpret_cast<unsigned *>(p) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) |
                                           ((unsigned)v[3] << 24);
    } else {
        for (int j = 0; j < m; ++j) p[j] = v[j];
    }
}
__host__ __device__ __forceinline__ void resize_store4(float *p, int m, const float v[4]) {
    if (m == 4 && (((uintptr_t)p) & 15) == 0) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < m; ++j) p[j] = v[j];
    }
}

// Thread t's share of the vertical pass: strip[r][q] = the four tap rows of output row r at window
// element q (q along x * C from column c0; wwc elements, row stride S), four elements per item.
template <typename T>
__host__ __device__ __forceinline__ void resize_vpass(int t, const ResizeArgs &A, const ResizeTile &L, const T *img,
                                                      int th, int c0, int wwc, int S, double *strip) {
    const int ng = (wwc + 3) >> 2;
    for (int g = t; g < th * ng; g += RT) {
        const int r = g / ng, q4 = (g - r * ng) * 4;
        const int m = wwc - q4 < 4 ? wwc - q4 : 4;
        double a[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) resize_load4(img + ((long)L.iy[r * 4 + k] * A.wi + c0) * A.C + q4, m, a[k]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < m) strip[r * S + q4 + j] = resize_tap4(&L.wy[r * 4], a[0][j], a[1][j], a[2][j], a[3][j]);
    }
}

// Thread t's share of the horizontal pass: four output elements of one tile row per item, each a
// 4-tap gather from the strip.  orow: the tile's first output element.
template <typename T>
__host__ __device__ __forceinline__ void resize_hpass(int t, const ResizeArgs &A, const ResizeTile &L, T *orow, int th,
                                                      int tw, int c0, int S, const double *strip) {
    const int twc = tw * A.C, ng = (twc + 3) >> 2;
    const long ostride = (long)A.wo * A.C;
    for (int g = t; g < th * ng; g += RT) {
        const int r = g / ng, q4 = (g - r * ng) * 4;
        const int m = twc - q4 < 4 ? twc - q4 : 4;
        T v[4] = {};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= m) continue;
            const int o = (q4 + j) / A.C, c = (q4 + j) - o * A.C;
            const double *s = strip + r * S + c;
            const int *ix = &L.ix[o * 4];
            const double h = resize_tap4(&L.wx[o * 4], s[(ix[0] - c0) * A.C], s[(ix[1] - c0) * A.C],
                                         s[(ix[2] - c0) * A.C], s[(ix[3] - c0) * A.C]);
            v[j] = resize_cvt(h, A, T());
        }
        resize_store4(orow + r * ostride + q4, m, v);
    }
}

// The same values without the strip, for a tile whose window does not fit it (a steep downscale, a
// large C): every output element runs its four vertical passes itself.
template <typename T>
__host__ __device__ __forceinline__ void resize_direct(int t, const ResizeArgs &A, const ResizeTile &L, const T *img,
                                                       T *orow, int th, int tw) {
    const int twc = tw * A.C;
    const long ostride = (long)A.wo * A.C;
    for (int e = t; e < th * twc; e += RT) {
        const int r = e / twc, q = e - r * twc;
        const int o = q / A.C, c = q - o * A.C;
        const int *iy = &L.iy[r * 4];
        double tk[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const T *p = img + (long)L.ix[o * 4 + k] * A.C + c;
            const long rs = (long)A.wi * A.C;
            tk[k] = resize_tap4(&L.wy[r * 4], (double)p[iy[0] * rs], (double)p[iy[1] * rs], (double)p[iy[2] * rs],
                                (double)p[iy[3] * rs]);
        }
        orow[r * ostride + q] = resize_cvt(resize_tap4(&L.wx[o * 4], tk[0], tk[1], tk[2], tk[3]), A, T());
    }
}

// doubles of strip row stride for a window of wwc elements: odd, so that lanes of different rows
// gather from different banks; 0 when RTH rows of it do not fit
__host__ __device__ __forceinline__ int resize_stride(long wwc) {
    const long S = wwc | 1;
    return S * RTH <= RCAP ? (int)S : 0;
}

// grid (tiles along h, tiles along w, n)
template <typename T>
__global__ void __launch_bounds__(RT)
k_resize(ResizeArgs A, const T *__restrict__ in, T *__restrict__ out, const int *__restrict__ iy,
         const double *__restrict__ wy, const int *__restrict__ ix, const double *__restrict__ wx) {
    __shared__ ResizeTile L;
    __shared__ double strip[RCAP];
    __shared__ int win[2];   // first and last input column of the tile's taps
    const int t = threadIdx.x;
    const int oy0 = blockIdx.x * RTH, ox0 = blockIdx.y * RTW;
    const int th = min(RTH, A.ho - oy0), tw = min(RTW, A.wo - ox0);
    if (t == 0) {
        win[0] = A.wi - 1;
        win[1] = 0;
    }
    __syncthreads();
    int lo = A.wi - 1, hi = 0;
    if (t < tw * 4) {
        lo = hi = L.ix[t] = min(max(ix[(long)ox0 * 4 + t], 0), A.wi - 1);
        L.wx[t] = wx[(long)ox0 * 4 + t];
    }
    if (t < th * 4) {
        L.iy[t] = min(max(iy[(long)oy0 * 4 + t], 0), A.hi - 1);
        L.wy[t] = wy[(long)oy0 * 4 + t];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if ((t & 63) == 0) {
        atomicMin(&win[0], lo);
        atomicMax(&win[1], hi);
    }
    __syncthreads();
    const int c0 = win[0];
    const long wwc = (long)(win[1] - c0 + 1) * A.C;
    const int S = resize_stride(wwc);
    const T *img = in + (long)blockIdx.z * A.hi * A.wi * A.C;
    T *orow = out + (((long)blockIdx.z * A.ho + oy0) * A.wo + ox0) * A.C;
    if (S) {
        resize_vpass(t, A, L, img, th, c0, (int)wwc, S, strip);
        __syncthreads();
        resize_hpass(t, A, L, orow, th, tw, c0, S, strip);
    } else {
        resize_direct(t, A, L, img, orow, th, tw);
    }
}

template <typename T>
static int resize_launch(const char *name, int n, int hi, int wi, int C, int ho, int wo, const T *in, T *out,
                         const int *iy, const double *wy, const int *ix, const double *wx, double mul, double bias,
                         hipStream_t stream) {
    const int lim = 1 << 20;   // (the grid's limits; element offsets stay far inside 64 bits)
    DG_ARG(n >= 0 && n <= 65535 && hi >= 1 && wi >= 1 && ho >= 1 && wo >= 1 && C >= 1 && hi <= lim && wi <= lim &&
               ho <= lim && wo <= lim && C <= 4096 && (long)hi * wi <= (1L << 34) && (long)ho * wo <= (1L << 34),
           "%s: bad shape: n %d, %dx%d -> %dx%d, C %d", name, n, hi, wi, ho, wo, C);
    DG_ARG(std::isfinite(mul) && std::isfinite(bias), "%s: mul and bias must be finite", name);
    if (n == 0) return DG_OK;
    DG_ARG(in && out && iy && wy && ix && wx, "%s: NULL tensor", name);
    DG_ARG((const void *)in != (const void *)out, "%s: in and out are the same buffer", name);
    DG_ARG(((((uintptr_t)iy) | ((uintptr_t)ix)) & 3) == 0 && ((((uintptr_t)wy) | ((uintptr_t)wx)) & 7) == 0,
           "%s: misaligned tap tables", name);
    ResizeArgs A;
    A.hi = hi; A.wi = wi; A.C = C; A.ho = ho; A.wo = wo;
    A.mul = mul; A.bias = bias;
    hipLaunchKernelGGL(k_resize<T>, dim3(dg_cdiv(ho, RTH), dg_cdiv(wo, RTW), n), dim3(RT), 0, stream, A, in, out, iy, wy,
                       ix, wx);
    DG_LAUNCHED(name);
    return DG_OK;
}

}  // namespace dg

int dg_resize_u8(int n, int hi, int wi, int C, int ho, int wo, const unsigned char *in, unsigned char *out,
                 const int *iy, const double *wy, const int *ix, const double *wx, double mul, double bias,
                 dg_stream_t stream) {
    return dg::resize_launch("resize_u8", n, hi, wi, C, ho, wo, in, out, iy, wy, ix, wx, mul, bias, (hipStream_t)stream);
}

int dg_resize_f32(int n, int hi, int wi, int C, int ho, int wo, const float *in, float *out, const int *iy,
                  const double *wy, const int *ix, const double *wx, dg_stream_t stream) {
    return dg::resize_launch("resize_f32", n, hi, wi, C, ho, wo, in, out, iy, wy, ix, wx, 1.0, 0.0, (hipStream_t)stream);
}
