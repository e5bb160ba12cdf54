// Image inference kernels: BatchNorm folding into conv weights, and the uint8 <-> fp32 tile
// staging around the generator forward (the reference's infer.py / infer_video.py:138-159).
#include "common.h"
#include <algorithm>
#include <cstdlib>

namespace dg {

static unsigned infer_grid(long n) { return (unsigned)std::max<long>(1, std::min<long>(dg_cdiv(n, 256), 8192)); }

// s = gamma / sqrt(var + eps), each step one correctly rounded fp32 operation
__device__ __forceinline__ float bn_scale(float gamma, float var, float eps) { return gamma / sqrtf(var + eps); }

// w [taps][Cin][Cout] (Conv2D) or [taps][Cout][Cin] (Conv2DTranspose): w_out = w * s[co];
// bias_out[co] = beta + (bias_in - mean) * s.  vec: float4 groups that share the layout's
// alignment (total % 4 == 0, 16-byte aligned pointers; Cout % 4 == 0, or Cin % 4 == 0 transposed)
__global__ void __launch_bounds__(256)
k_bn_fold(long total, int Cin, int Cout, int transpose, const float *__restrict__ w, const float *__restrict__ gamma,
          const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ var, float eps,
          const float *__restrict__ bias_in, float *__restrict__ w_out, float *__restrict__ bias_out, int vec) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long c = gid; c < Cout; c += stride) {
        const float s = bn_scale(gamma[c], var[c], eps);
        const float m = bias_in ? bias_in[c] - mean[c] : -mean[c];
        bias_out[c] = m * s + beta[c];
    }
    if (vec) {
        const long n4 = total >> 2;
        for (long i = gid; i < n4; i += stride) {
            const long e = i << 2;
            f32x4 v = reinterpret_cast<const f32x4 *>(w)[i];
            if (transpose) {
                const int co = (int)((e / Cin) % Cout);
                v *= bn_scale(gamma[co], var[co], eps);
            } else {
                const int co = (int)(e % Cout);
                const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + co);
                const f32x4 vr = *reinterpret_cast<const f32x4 *>(var + co);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] *= bn_scale(g[q], vr[q], eps);
            }
            reinterpret_cast<f32x4 *>(w_out)[i] = v;
        }
        return;
    }
    for (long e = gid; e < total; e += stride) {
        const int co = transpose ? (int)((e / Cin) % Cout) : (int)(e % Cout);
        w_out[e] = w[e] * bn_scale(gamma[co], var[co], eps);
    }
}

// ---- uint8 image <-> fp32 tiles --------------------------------------------------------------
struct TileGeom {
    int n, h, w;      // images [n][h][w][3]
    int Th, Tw;       // tile
    int Sh, Sw;       // stride between tile origins
    int oy, ox;       // image row / column of tile (0, 0)'s first pixel
    int gi, gj;       // tiles per image
};

constexpr int PXG = 16;   // pixels per thread: 48 B of uint8, 12 float4

// the source index of image coordinate r (size h): -1 = the constant pad; reflect as
// np.pad(mode="reflect") for any pad width
__device__ __forceinline__ int pad_index(int r, int h, int pad) {
    if ((unsigned)r < (unsigned)h) return r;
    if (pad == DG_PAD_BLACK) return -1;
    if (h == 1) return 0;
    const int p = 2 * (h - 1);
    int j = r % p;
    if (j < 0) j += p;
    return j >= h ? p - j : j;
}

// infer_video.py:139-143: convert_image_dtype(u8, float32) = u8 * (1 / 255), then * 2 - 1
__device__ __forceinline__ float u8_to_unit(unsigned b) { return ((float)b * (1.0f / 255.0f)) * 2.0f - 1.0f; }
// infer_video.py:149-159: clip(v * 0.5 + 0.5, 0, 1) * 255 to uint8, rounded to nearest (+ 0.5, then
// truncated: tf.image.convert_image_dtype's rule) where the reference truncates -- the chain above
// rounds a * 2 - 1 at the spacing of 1.0, so truncation would return 47 of the 256 byte values one
// level darker through an identity network.  NaN -> 0: fmaxf drops it.  The product and the sum
// are two roundings (no FMA), as numpy evaluates them.
__device__ __forceinline__ unsigned unit_to_u8(float v) {
    const float t = fminf(fmaxf(v * 0.5f + 0.5f, 0.0f), 1.0f);
    return (unsigned)__fadd_rn(__fmul_rn(t, 255.0f), 0.5f);
}

__global__ void __launch_bounds__(256)
k_u8_stage(TileGeom g, int pad, const unsigned char *__restrict__ img, float *__restrict__ tiles) {
    const int gpr = (g.Tw + PXG - 1) / PXG;   // pixel groups per tile row
    const long total = (long)g.n * g.gi * g.gj * g.Th * gpr;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int gx = (int)(e % gpr);
        long q = e / gpr;
        const int ty = (int)(q % g.Th);
        const long t = q / g.Th;               // tile: (image * gi + i) * gj + j
        const int j = (int)(t % g.gj);
        const int i = (int)((t / g.gj) % g.gi);
        const int im = (int)(t / ((long)g.gi * g.gj));
        const int rr = pad_index(g.oy + i * g.Sh + ty, g.h, pad);
        const int c0 = g.ox + j * g.Sw + gx * PXG;
        const int npx = min(PXG, g.Tw - gx * PXG);
        float v[3 * PXG];
        const unsigned char *row = img + ((long)im * g.h + max(rr, 0)) * g.w * 3;
        if (rr >= 0 && npx == PXG && c0 >= 0 && c0 + PXG <= g.w) {
            // 48 contiguous bytes of one image row
            const unsigned char *src = row + (long)c0 * 3;
            unsigned wd[12];
            if ((((uintptr_t)src) & 15) == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint4 u = reinterpret_cast<const uint4 *>(src)[k];
                    wd[4 * k] = u.x; wd[4 * k + 1] = u.y; wd[4 * k + 2] = u.z; wd[4 * k + 3] = u.w;
                }
            } else if ((((uintptr_t)src) & 3) == 0) {
#pragma unroll
                for (int k = 0; k < 12; ++k) wd[k] = reinterpret_cast<const unsigned *>(src)[k];
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    wd[k] = (unsigned)src[4 * k] | ((unsigned)src[4 * k + 1] << 8) | ((unsigned)src[4 * k + 2] << 16) |
                            ((unsigned)src[4 * k + 3] << 24);
            }
#pragma unroll
            for (int k = 0; k < 3 * PXG; ++k) v[k] = u8_to_unit((wd[k >> 2] >> (8 * (k & 3))) & 255u);
        } else {
#pragma unroll
            for (int px = 0; px < PXG; ++px) {
                const int cc = (rr >= 0 && px < npx) ? pad_index(c0 + px, g.w, pad) : -1;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[3 * px + c] = cc >= 0 ? u8_to_unit(row[(long)cc * 3 + c]) : -1.0f;
            }
        }
        float *dst = tiles + ((t * g.Th + ty) * g.Tw + (long)gx * PXG) * 3;
        if (npx == PXG && (((uintptr_t)dst) & 15) == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                reinterpret_cast<f32x4 *>(dst)[k] = f32x4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
        } else {
#pragma unroll
            for (int k = 0; k < 3 * PXG; ++k)
                if (k < 3 * npx) dst[k] = v[k];
        }
    }
}

// output pixel (y, x) of image im comes from tile (i, j), i = clamp((y - oy - mt) / Sh, 0, gi - 1)
// (the tile whose interior [mt, mt + Sh) holds it), tile row y - (oy + i * Sh)
__global__ void __launch_bounds__(256)
k_u8_unstage(TileGeom g, int mt, int ml, const float *__restrict__ tiles, unsigned char *__restrict__ out) {
    const int gpr = (g.w + PXG - 1) / PXG;
    const long total = (long)g.n * g.h * gpr;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int gx = (int)(e % gpr);
        const long q = e / gpr;
        const int y = (int)(q % g.h);
        const int im = (int)(q / g.h);
        const int i = min(max((y - g.oy - mt) / g.Sh, 0), g.gi - 1);
        const int ty = y - (g.oy + i * g.Sh);
        const int x0 = gx * PXG;
        const int npx = min(PXG, g.w - x0);
        const long trow = (((long)im * g.gi + i) * g.gj * g.Th + ty) * g.Tw;   // tile (i, 0)'s row ty
        auto tile_col = [&](int x, long &base) {
            const int j = min(max((x - g.ox - ml) / g.Sw, 0), g.gj - 1);
            base = trow + (long)j * g.Th * g.Tw;
            return x - (g.ox + j * g.Sw);
        };
        float v[3 * PXG];
        long b0, b1;
        const int tx0 = tile_col(x0, b0);
        (void)tile_col(x0 + npx - 1, b1);
        if (npx == PXG && b0 == b1) {
            const float *src = tiles + (b0 + tx0) * 3;
            if ((((uintptr_t)src) & 15) == 0) {
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    const f32x4 u = reinterpret_cast<const f32x4 *>(src)[k];
                    v[4 * k] = u[0]; v[4 * k + 1] = u[1]; v[4 * k + 2] = u[2]; v[4 * k + 3] = u[3];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3 * PXG; ++k) v[k] = src[k];
            }
        } else {
#pragma unroll
            for (int px = 0; px < PXG; ++px) {
                long b;
                const int tx = tile_col(x0 + min(px, npx - 1), b);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[3 * px + c] = tiles[(b + tx) * 3 + c];
            }
        }
        unsigned wd[12];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            wd[k] = unit_to_u8(v[4 * k]) | (unit_to_u8(v[4 * k + 1]) << 8) | (unit_to_u8(v[4 * k + 2]) << 16) |
                    (unit_to_u8(v[4 * k + 3]) << 24);
        unsigned char *dst = out + (((long)im * g.h + y) * g.w + x0) * 3;
        if (npx == PXG && (((uintptr_t)dst) & 15) == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                reinterpret_cast<uint4 *>(dst)[k] = uint4{wd[4 * k], wd[4 * k + 1], wd[4 * k + 2], wd[4 * k + 3]};
        } else if (npx == PXG && (((uintptr_t)dst) & 3) == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) reinterpret_cast<unsigned *>(dst)[k] = wd[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3 * PXG; ++k)
                if (k < 3 * npx) dst[k] = (unsigned char)((wd[k >> 2] >> (8 * (k & 3))) & 255u);
        }
    }
}

static bool tile_geom_ok(const TileGeom &g) {
    return g.n >= 0 && g.h >= 1 && g.w >= 1 && g.Th >= 1 && g.Tw >= 1 && g.Sh >= 1 && g.Sw >= 1 && g.gi >= 1 &&
           g.gj >= 1 && (long)g.gi * g.Sh + g.Th < (1L << 30) && (long)g.gj * g.Sw + g.Tw < (1L << 30) &&
           std::abs((long)g.oy) < (1L << 30) && std::abs((long)g.ox) < (1L << 30);
}

}  // namespace dg

int dg_bn_fold(int taps, int Cin, int Cout, int transpose, const float *w, const float *gamma, const float *beta,
               const float *moving_mean, const float *moving_var, float eps, const float *bias_in, float *w_out,
               float *bias_out, dg_stream_t stream) {
    DG_ARG(taps >= 1 && Cin >= 1 && Cout >= 1, "bad shape: taps %d Cin %d Cout %d", taps, Cin, Cout);
    DG_ARG(w && gamma && beta && moving_mean && moving_var && w_out && bias_out, "NULL tensor");
    DG_ARG(eps > 0.f, "eps must be positive");
    const long total = (long)taps * Cin * Cout;
    const bool aligned = ((((uintptr_t)w) | ((uintptr_t)w_out) | ((uintptr_t)gamma) | ((uintptr_t)moving_var)) & 15) == 0;
    const int vec = aligned && total % 4 == 0 && (transpose ? Cin % 4 == 0 : Cout % 4 == 0);
    hipLaunchKernelGGL(dg::k_bn_fold, dim3(dg::infer_grid(vec ? total / 4 : total)), dim3(256), 0, (hipStream_t)stream,
                       total, Cin, Cout, transpose ? 1 : 0, w, gamma, beta, moving_mean, moving_var, eps, bias_in, w_out,
                       bias_out, vec);
    DG_LAUNCHED("bn_fold");
    return DG_OK;
}

int dg_u8_stage(int n, int h, int w, int Th, int Tw, int Sh, int Sw, int oy, int ox, int gi, int gj, int pad,
                const unsigned char *img, float *tiles, dg_stream_t stream) {
    const dg::TileGeom g{n, h, w, Th, Tw, Sh, Sw, oy, ox, gi, gj};
    DG_ARG(dg::tile_geom_ok(g), "bad tile geometry");
    DG_ARG(pad == DG_PAD_BLACK || pad == DG_PAD_REFLECT, "pad is DG_PAD_BLACK or DG_PAD_REFLECT");
    DG_ARG((img && tiles) || n == 0, "NULL tensor");
    if (n == 0) return DG_OK;
    const long total = (long)n * gi * gj * Th * ((Tw + dg::PXG - 1) / dg::PXG);
    hipLaunchKernelGGL(dg::k_u8_stage, dim3(dg::infer_grid(total)), dim3(256), 0, (hipStream_t)stream, g, pad, img,
                       tiles);
    DG_LAUNCHED("u8_stage");
    return DG_OK;
}

int dg_u8_unstage(int n, int h, int w, int Th, int Tw, int Sh, int Sw, int oy, int ox, int gi, int gj, int margin_top,
                  int margin_left, const float *tiles, unsigned char *out, dg_stream_t stream) {
    const dg::TileGeom g{n, h, w, Th, Tw, Sh, Sw, oy, ox, gi, gj};
    DG_ARG(dg::tile_geom_ok(g), "bad tile geometry");
    // every output pixel reads inside its tile: y - oy - margin >= 0 so the tile index never clamps
    // from below, an unclamped index gives a tile row in [margin, margin + S), and the last
    // tile (the clamp from above) must reach the image's last row / column
    DG_ARG(margin_top >= 0 && margin_left >= 0 && margin_top + Sh <= Th && margin_left + Sw <= Tw,
           "the tile interior [margin, margin + stride) must lie inside the tile");
    DG_ARG(oy + margin_top <= 0 && ox + margin_left <= 0, "the first tile's interior must start at or before pixel 0");
    DG_ARG((long)h - 1 - oy - (long)(gi - 1) * Sh < Th && (long)w - 1 - ox - (long)(gj - 1) * Sw < Tw,
           "the tile grid does not cover the image");
    DG_ARG((tiles && out) || n == 0, "NULL tensor");
    if (n == 0) return DG_OK;
    const long total = (long)n * h * ((w + dg::PXG - 1) / dg::PXG);
    hipLaunchKernelGGL(dg::k_u8_unstage, dim3(dg::infer_grid(total)), dim3(256), 0, (hipStream_t)stream, g, margin_top,
                       margin_left, tiles, out);
    DG_LAUNCHED("u8_unstage");
    return DG_OK;
}
