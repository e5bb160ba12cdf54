// Super-resolution inference kernels (dgan/sr_infer.py): the depthwise conv with a fused
// activation (a BN-folded DepthwiseConv2D -> ReLU) and the fused inverted-residual block of the
// FastSRGAN generator (fsrgan.py:112-177 with its BatchNorms folded):
//   y = b_proj + W_proj^T relu(b_dw + dw3x3_same(mask relu(b_exp + W_exp^T x))) [+ res]
// whose expanded tensors never leave the chip.
#include "common.h"
#include <algorithm>

namespace dg {

// --------------------------------------------------------------------------
// DepthwiseConv2D(3x3, 'same') + bias + activation: k_dw_rows<false> of layers.hip (same block
// geometry, same tap order, s + bias) with act applied to the sum -- with DG_ACT_NONE the
// result is dg_dwconv3_fwd's bit for bit, with an activation that of dg_act_fwd after it.
// --------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_dw_rows_act(int N, int H, int W, int C, const float *__restrict__ src, int lds, const float *__restrict__ k,
              const float *__restrict__ b, float *__restrict__ dst, int ldd, int act, float alpha, int RB, int nrc) {
    const int cl = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int w = blockIdx.y * 4 + wv;
    if (c >= C || w >= W) return;
    const int n = blockIdx.z / nrc, rc = blockIdx.z - n * nrc;
    const int h0 = rc * RB, h1 = min(H, h0 + RB);
    float kk[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) kk[q] = k[q * C + c];
    const float bias = b ? b[c] : 0.f;
    const bool okl = w > 0, okr = w + 1 < W;
    const float *sb = src + (long)n * H * W * lds + c;
    float *db = dst + (long)n * H * W * ldd + c;
    auto ld3 = [&](int h, float &v0, float &v1, float &v2) {
        const bool okh = h >= 0 && h < H;
        const float *r = sb + ((long)h * W + w) * lds;
        v0 = okh && okl ? r[-lds] : 0.f;
        v1 = okh ? r[0] : 0.f;
        v2 = okh && okr ? r[lds] : 0.f;
    };
    float u0, u1, u2, m0, m1, m2;
    ld3(h0 - 1, u0, u1, u2);
    ld3(h0, m0, m1, m2);
    for (int h = h0; h < h1; ++h) {
        float d0, d1, d2;
        ld3(h + 1, d0, d1, d2);
        float s = 0.f;
        s = fmaf(u0, kk[0], s); s = fmaf(u1, kk[1], s); s = fmaf(u2, kk[2], s);
        s = fmaf(m0, kk[3], s); s = fmaf(m1, kk[4], s); s = fmaf(m2, kk[5], s);
        s = fmaf(d0, kk[6], s); s = fmaf(d1, kk[7], s); s = fmaf(d2, kk[8], s);
        db[((long)h * W + w) * ldd] = act_fwd(s + bias, act, alpha);
        u0 = m0; u1 = m1; u2 = m2;
        m0 = d0; m1 = d1; m2 = d2;
    }
}

// --------------------------------------------------------------------------
// The fused inverted-residual block, C = Co = 32, E a multiple of 32 up to 192.
//
// One workgroup (4 waves) owns a 16 x 16 output tile of one image.  Its 18 x 18 halo of x
// lives in registers for the whole kernel, already in the MFMA operand form: halo pixels are
// numbered p = row * 18 + col and cut into 11 groups of 32 (the last one part empty); wave v
// owns groups v, v + 4, v + 8, and lane (p & 31, half) holds channels 16 half .. 16 half + 15
// of its pixel -- 64 contiguous bytes of global memory.  Per chunk of 32 expanded channels:
//
//   expand    D[e][p] = b_exp[e] + sum_c W_exp[c][e] x[p][c]: v_mfma_f32_32x32x2_f32 with
//             A = W_exp^T (the lane's column e, 16 registers per chunk) and B = x; step s of 16
//             sums channels s (lane half 0) and 16 + s (half 1) -- the k order is free as long
//             as both operands use it.  A lane then holds its pixel's 16 channels
//             8g + 4 half + (0..3): ReLU, zeroed when the pixel lies outside the image (the
//             border rule: Keras pads the depthwise INPUT with zeros), four 16-byte LDS writes.
//   barrier
//   depthwise lane (q & 31, half) of output-pixel group q >> 5 (wave v: groups v, v + 4)
//             computes channels 16 half .. + 15 of its pixel from nine 64-byte LDS reads, taps
//             and bias from an LDS copy of k_dw; ReLU.  Those 16 registers ARE the B operand
//   project   of D[co][q] += sum_e W_proj[e][co] dw[q][e], accumulated over the chunks in 2 x 16
//             registers.
//   barrier   (the next chunk's expand overwrites the LDS image)
//
// LDS: the expanded chunk [324 pixels][36 floats] = 46,656 B + k_dw and b_dw [10][E] <= 7,680 B:
// 54,336 B, room for three workgroups per CU; the registers (193 VGPRs: the halo 48, the project
// accumulators 32, both weight operands 32, the depthwise sums 32) allow two.  The pixel stride of 36 floats (144 B) puts the 16 lanes
// of every ds_read_b128 / ds_write_b128 group whose pixels differ mod 16 on 16 different 16-byte
// slots of the 256-byte bank row (36 p mod 64 takes 16 distinct multiples of 4).
// --------------------------------------------------------------------------
constexpr int MB_T = 16;                     // output tile edge
constexpr int MB_HT = MB_T + 2;              // halo tile edge
constexpr int MB_HP = MB_HT * MB_HT;         // halo pixels
constexpr int MB_C = 32;                     // C = Co = expanded channels per chunk
constexpr int MB_LD = 36;                    // LDS pixel stride, floats
constexpr int MB_EMAX = 192;
constexpr int MB_XG = (MB_HP + 31) / 32;     // halo pixel groups: 11
constexpr int MB_XW = (MB_XG + 3) / 4;       // per wave: 3
constexpr int MB_QW = MB_T * MB_T / 32 / 4;  // output pixel groups per wave: 2

__global__ void __launch_bounds__(256, 2)
k_mbconv(int H, int W, int E, const float *__restrict__ x, int ldx, const float *__restrict__ we,
         const float *__restrict__ be, const float *__restrict__ kd, const float *__restrict__ bd,
         const float *__restrict__ wp, const float *__restrict__ bp, const float *res, int ldr, float *y, int ldy) {
    __shared__ __attribute__((aligned(16))) float s_exp[MB_HP * MB_LD];
    __shared__ __attribute__((aligned(16))) float s_kd[10 * MB_EMAX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int th0 = blockIdx.y * MB_T, tw0 = blockIdx.x * MB_T;
    const long img = (long)blockIdx.z * H * W;

    for (int i = tid; i < 9 * E; i += 256) s_kd[i] = kd[i];
    for (int i = tid; i < E; i += 256) s_kd[9 * E + i] = bd ? bd[i] : 0.f;

    // the halo of x, as the expand GEMM's B operand
    float xb[MB_XW][16];
    bool inimg[MB_XW];
#pragma unroll
    for (int k = 0; k < MB_XW; ++k) {
        const int p = 32 * (wv + 4 * k) + l31;
        const int gh = th0 - 1 + p / MB_HT, gw = tw0 - 1 + p % MB_HT;
        inimg[k] = p < MB_HP && gh >= 0 && gh < H && gw >= 0 && gw < W;
        const float *px = x + (img + (long)gh * W + gw) * ldx + 16 * hh;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (inimg[k]) v = *reinterpret_cast<const f32x4 *>(px + 4 * m);
#pragma unroll
            for (int u = 0; u < 4; ++u) xb[k][4 * m + u] = v[u];
        }
    }

    f32x16 pacc[MB_QW];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float b = bp ? bp[8 * (r >> 2) + 4 * hh + (r & 3)] : 0.f;
#pragma unroll
        for (int k = 0; k < MB_QW; ++k) pacc[k][r] = b;
    }

    for (int e0 = 0; e0 < E; e0 += MB_C) {
        float wE[16], wP[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            wE[s] = we[(long)(16 * hh + s) * E + e0 + l31];
            wP[s] = wp[(long)(e0 + 16 * hh + s) * MB_C + l31];
        }
        f32x16 bexp;
#pragma unroll
        for (int r = 0; r < 16; ++r) bexp[r] = be ? be[e0 + 8 * (r >> 2) + 4 * hh + (r & 3)] : 0.f;

        // expand -> LDS
#pragma unroll
        for (int k = 0; k < MB_XW; ++k) {
            if (wv + 4 * k >= MB_XG) continue;   // (wave-uniform)
            f32x16 acc = bexp;
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wE[s], xb[k][s], acc, 0, 0, 0);
            const int p = 32 * (wv + 4 * k) + l31;
            if (p < MB_HP) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = inimg[k] ? fmaxf(acc[4 * g + u], 0.f) : 0.f;
                    *reinterpret_cast<f32x4 *>(&s_exp[p * MB_LD + 8 * g + 4 * hh]) = v;
                }
            }
        }
        __syncthreads();   // (the first pass: s_kd too)

        // depthwise 3x3 out of LDS, then the project GEMM
        float d[MB_QW][16];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const f32x4 b4 = *reinterpret_cast<const f32x4 *>(&s_kd[9 * E + e0 + 16 * hh + 4 * m]);
#pragma unroll
            for (int k = 0; k < MB_QW; ++k)
#pragma unroll
                for (int u = 0; u < 4; ++u) d[k][4 * m + u] = b4[u];
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x4 w4 = *reinterpret_cast<const f32x4 *>(&s_kd[t * E + e0 + 16 * hh + 4 * m]);
#pragma unroll
                for (int k = 0; k < MB_QW; ++k) {
                    const int q = 32 * (wv + 4 * k) + l31;
                    const int hp = ((q >> 4) + t / 3) * MB_HT + (q & 15) + t % 3;
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(&s_exp[hp * MB_LD + 16 * hh + 4 * m]);
#pragma unroll
                    for (int u = 0; u < 4; ++u) d[k][4 * m + u] = fmaf(v[u], w4[u], d[k][4 * m + u]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < MB_QW; ++k)
#pragma unroll
            for (int s = 0; s < 16; ++s)
                pacc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(wP[s], fmaxf(d[k][s], 0.f), pacc[k], 0, 0, 0);
        __syncthreads();
    }

    // y = project (+ res): lane (q & 31, half) holds channels 8g + 4 half + (0..3) of its pixel
#pragma unroll
    for (int k = 0; k < MB_QW; ++k) {
        const int q = 32 * (wv + 4 * k) + l31;
        const int gh = th0 + (q >> 4), gw = tw0 + (q & 15);
        if (gh >= H || gw >= W) continue;
        const long pix = img + (long)gh * W + gw;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = 8 * g + 4 * hh;
            f32x4 v = {pacc[k][4 * g], pacc[k][4 * g + 1], pacc[k][4 * g + 2], pacc[k][4 * g + 3]};
            if (res) v += *reinterpret_cast<const f32x4 *>(res + pix * ldr + co);
            *reinterpret_cast<f32x4 *>(y + pix * ldy + co) = v;
        }
    }
}

static bool mb_supported(int C, int E, int Co) {
    return C == MB_C && Co == MB_C && E >= MB_C && E <= MB_EMAX && E % MB_C == 0;
}

}  // namespace dg

int dg_dwconv3_fwd_act(int N, int H, int W, int C, const float *x, int ldx, const float *k, const float *bias,
                       int act, float alpha, float *y, int ldy, dg_stream_t stream) {
    DG_ARG(x && k && y, "NULL tensor");
    DG_ARG(N > 0 && H > 0 && W > 0 && C > 0 && ldx >= C && ldy >= C, "bad shape");
    DG_ARG(act >= DG_ACT_NONE && act <= DG_ACT_SIGMOID, "unknown activation %d", act);
    // (the row chunks of dg_dwconv3_fwd: >= 2048 blocks)
    const long cols = (long)dg_cdiv(C, 64) * dg_cdiv(W, 4) * N;
    const int want = (int)std::max<long>(1, std::min<long>(H, dg_cdiv(2048, cols)));
    const int RB = dg_cdiv(H, want), nrc = dg_cdiv(H, RB);
    DG_ARG((long)N * nrc <= 65535 && dg_cdiv(W, 4) <= 65535, "image too large for the launch grid");
    hipLaunchKernelGGL(dg::k_dw_rows_act, dim3(dg_cdiv(C, 64), dg_cdiv(W, 4), N * nrc), dim3(256), 0,
                       (hipStream_t)stream, N, H, W, C, x, ldx, k, bias, y, ldy, act, alpha, RB, nrc);
    DG_LAUNCHED("dwconv_fwd_act");
    return DG_OK;
}

int dg_mbconv_supported(int C, int E, int Co, int *ok) {
    DG_ARG(ok, "NULL argument");
    *ok = dg::mb_supported(C, E, Co) ? 1 : 0;
    return DG_OK;
}

int dg_mbconv_tile(int *tile) {
    DG_ARG(tile, "NULL argument");
    *tile = dg::MB_T;
    return DG_OK;
}

int dg_mbconv_fwd(int N, int H, int W, int C, int E, int Co, const float *x, int ldx, const float *w_exp,
                  const float *b_exp, const float *k_dw, const float *b_dw, const float *w_proj, const float *b_proj,
                  const float *res, int ldres, float *y, int ldy, dg_stream_t stream) {
    DG_ARG(dg::mb_supported(C, E, Co), "unsupported channel counts C %d E %d Co %d (C = Co = 32, E a multiple of 32 up to 192)",
           C, E, Co);
    DG_ARG(x && w_exp && k_dw && w_proj && y, "NULL tensor");
    DG_ARG(N > 0 && H > 0 && W > 0, "bad shape");
    DG_ARG(ldx >= C && ldy >= Co && ldx % 4 == 0 && ldy % 4 == 0 && (!res || (ldres >= Co && ldres % 4 == 0)),
           "pixel strides must be multiples of 4 floats and hold the channels");
    DG_ARG(((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)res)) & 15) == 0, "x, y and res must be 16-byte aligned");
    // neighbouring workgroups read x's halo after this one wrote y: the two may not share memory
    {
        const uintptr_t xs = (uintptr_t)x, ys = (uintptr_t)y;
        const uintptr_t npx = (uintptr_t)N * H * W;
        const uintptr_t xe = xs + ((npx - 1) * ldx + C) * sizeof(float), ye = ys + ((npx - 1) * ldy + Co) * sizeof(float);
        bool overlap = xs < ye && ys < xe;
        if (overlap && ldx == ldy) {
            // channel slices of one wider buffer are disjoint when their channel intervals are
            const uintptr_t ldb = (uintptr_t)ldx * sizeof(float);
            const uintptr_t d = ys >= xs ? (ys - xs) % ldb : (ldb - (xs - ys) % ldb) % ldb;   // y's offset in x's pixel
            overlap = !(d >= C * sizeof(float) && d + Co * sizeof(float) <= ldb);
        }
        DG_ARG(!overlap, "y may not alias x");
    }
    const unsigned gx = dg_cdiv(W, dg::MB_T), gy = dg_cdiv(H, dg::MB_T);
    DG_ARG(gy <= 65535 && N <= 65535, "image too large for the launch grid");
    hipLaunchKernelGGL(dg::k_mbconv, dim3(gx, gy, N), dim3(256), 0, (hipStream_t)stream, H, W, E, x, ldx, w_exp, b_exp,
                       k_dw, b_dw, w_proj, b_proj, res, ldres, y, ldy);
    DG_LAUNCHED("mbconv_fwd");
    return DG_OK;
}
