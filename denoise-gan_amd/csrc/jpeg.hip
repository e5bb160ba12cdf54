// JPEG round trip without the entropy coder (include/dgan.h "JPEG round trip"; the definition and
// the numpy reference with the same integer arithmetic: dgan/jpeg.py).  Two launches:
//   k_jpeg_blocks  a block per strip of four 16x16 MCUs: colour conversion and 4:2:0 downsampling
//                  into LDS, then the 24 blocks' forward DCT, quantise, dequantise and inverse DCT,
//                  one 8-point pass per lane over a row or column held in registers; the decoded
//                  Y, Cb and Cr go to uint8 planes in the workspace
//   k_jpeg_pixels  four output pixels of a row per thread: chroma upsampling from the planes (the
//                  triangle filter reads decoded chroma across block borders, hence the split) and
//                  the colour conversion back
// int32 throughout, no floating point.  The first kernel has read all of `in` before the second
// writes `out`, so the two may be one buffer.
#include "common.h"

namespace dg {

constexpr int JT = 192;             // threads of k_jpeg_blocks: one per block row, 24 blocks of 8
constexpr int JSW = 64, JSH = 16;   // luma pixels of a strip: four MCUs side by side
constexpr int JLD = 9;              // ints per block row in LDS: odd, so that the 32 lanes of a row
                                    // pass (stride JLD) and of a column pass (8 blocks x 8 columns)
                                    // each hit 32 different banks
constexpr int JBW = 64, JBH = 4;    // k_jpeg_pixels: a thread block covers 256 x 4 pixels
static_assert(JT == (JSW / 8) * (JSH / 8) * 8 * 3 / 2, "one lane per block row of the strip");

struct JpegTables {
    unsigned char t[128];   // luminance [64], chrominance [64], row-major
};

struct JpegArgs {
    int h, w, ch, cw;   // image, chroma plane
    int Hp, Wp;         // luma plane of the workspace: h, w rounded up to the strip
};

__host__ __device__ __forceinline__ long jpeg_image_bytes(int Hp, int Wp) { return (long)Hp * Wp / 2 * 3; }

#define JFIX(x) ((int)((x) * 65536.0 + 0.5))

__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// the rotations shared by the odd halves of both DCTs (jfdctint / jidctint, CONST_BITS 13)
__device__ __forceinline__ void jpeg_odd(int &t0, int &t1, int &t2, int &t3) {
    int z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
}

// one jfdctint pass in place: FIRST the row pass (output scaled by 4), else the column pass
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int d[8]) {
    const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
    int t4 = d[3] - d[4], t5 = d[2] - d[5], t6 = d[1] - d[6], t7 = d[0] - d[7];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15;
    const int z1 = (t12 + t13) * 4433;
    d[0] = FIRST ? (t10 + t11) * 4 : jpeg_descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : jpeg_descale(t10 - t11, 2);
    d[2] = jpeg_descale(z1 + t13 * 6270, n);
    d[6] = jpeg_descale(z1 - t12 * 15137, n);
    jpeg_odd(t4, t5, t6, t7);
    d[7] = jpeg_descale(t4, n);
    d[5] = jpeg_descale(t5, n);
    d[3] = jpeg_descale(t6, n);
    d[1] = jpeg_descale(t7, n);
}

// one jidctint pass in place: FIRST the column pass (descaled by 11), else the row pass (by 18)
template <bool FIRST>
__device__ __forceinline__ void jpeg_idct8(int c[8]) {
    const int z1 = (c[2] + c[6]) * 4433;
    const int t2 = z1 - c[6] * 15137, t3 = z1 + c[2] * 6270;
    const int t0 = (c[0] + c[4]) * 8192, t1 = (c[0] - c[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = c[7], a1 = c[5], a2 = c[3], a3 = c[1];
    jpeg_odd(a0, a1, a2, a3);
    constexpr int n = FIRST ? 11 : 18;
    c[0] = jpeg_descale(t10 + a3, n);
    c[7] = jpeg_descale(t10 - a3, n);
    c[1] = jpeg_descale(t11 + a2, n);
    c[6] = jpeg_descale(t11 - a2, n);
    c[2] = jpeg_descale(t12 + a1, n);
    c[5] = jpeg_descale(t12 - a1, n);
    c[3] = jpeg_descale(t13 + a0, n);
    c[4] = jpeg_descale(t13 - a0, n);
}

// libjpeg's range-limit table read at x & 1023
__device__ __forceinline__ unsigned jpeg_limit(int x) {
    x &= 1023;
    return x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896;
}

struct JpegYCC {
    int y, cb, cr;
};

__device__ __forceinline__ JpegYCC jpeg_ycc(const unsigned char *p) {
    const int r = p[0], g = p[1], b = p[2];
    JpegYCC v;
    v.y = (JFIX(.299) * r + JFIX(.587) * g + JFIX(.114) * b + 32768) >> 16;
    v.cb = (-JFIX(.16874) * r - JFIX(.33126) * g + JFIX(.5) * b + (128 << 16) + 32767) >> 16;
    v.cr = (JFIX(.5) * r - JFIX(.41869) * g - JFIX(.08131) * b + (128 << 16) + 32767) >> 16;
    return v;
}

// grid (strips along w, strips along h, n)
__global__ void __launch_bounds__(JT)
k_jpeg_blocks(JpegArgs A, JpegTables Q, const unsigned char *__restrict__ in, unsigned char *__restrict__ ws) {
    __shared__ int buf[JT * JLD];   // block row R = block * 8 + row at R * JLD; blocks: 16 Y (2 x 8), 4 Cb, 4 Cr
    __shared__ int qt[128];
    const int t = threadIdx.x;
    const int X0 = blockIdx.x * JSW, Y0 = blockIdx.y * JSH;
    const unsigned char *img = in + (long)blockIdx.z * A.h * A.w * 3;
    if (t < 128) qt[t] = Q.t[t];

    // colour conversion and downsampling, a 2x2 quad per item; coordinates clamp into the image
    // (edge replication), the chroma rows below the image repeat the last chroma row
    for (int q = t; q < (JSW / 2) * (JSH / 2); q += JT) {
        const int qx = q & (JSW / 2 - 1), qy = q / (JSW / 2);
        const int x0 = min(X0 + 2 * qx, A.w - 1), x1 = min(X0 + 2 * qx + 1, A.w - 1);
        const int gy = Y0 + 2 * qy;
        const int y0 = min(gy, A.h - 1), y1 = min(gy + 1, A.h - 1);
        const JpegYCC p00 = jpeg_ycc(img + ((long)y0 * A.w + x0) * 3), p01 = jpeg_ycc(img + ((long)y0 * A.w + x1) * 3);
        const JpegYCC p10 = jpeg_ycc(img + ((long)y1 * A.w + x0) * 3), p11 = jpeg_ycc(img + ((long)y1 * A.w + x1) * 3);
        const int ly = 2 * qy, lx = 2 * qx;
        int *yrow = buf + (((ly >> 3) * 8 + (lx >> 3)) * 8 + (ly & 7)) * JLD + (lx & 7);
        yrow[0] = p00.y - 128;
        yrow[1] = p01.y - 128;
        yrow[JLD] = p10.y - 128;
        yrow[JLD + 1] = p11.y - 128;
        int cb = p00.cb + p01.cb + p10.cb + p11.cb, cr = p00.cr + p01.cr + p10.cr + p11.cr;
        if ((gy >> 1) >= A.ch) {
            const int r0 = 2 * A.ch - 2, r1 = min(2 * A.ch - 1, A.h - 1);
            const JpegYCC c00 = jpeg_ycc(img + ((long)r0 * A.w + x0) * 3), c01 = jpeg_ycc(img + ((long)r0 * A.w + x1) * 3);
            const JpegYCC c10 = jpeg_ycc(img + ((long)r1 * A.w + x0) * 3), c11 = jpeg_ycc(img + ((long)r1 * A.w + x1) * 3);
            cb = c00.cb + c01.cb + c10.cb + c11.cb;
            cr = c00.cr + c01.cr + c10.cr + c11.cr;
        }
        const int bias = 1 + (qx & 1);
        int *crow = buf + ((16 + (qx >> 3)) * 8 + qy) * JLD + (qx & 7);
        crow[0] = ((cb + bias) >> 2) - 128;
        crow[4 * 8 * JLD] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();

    int d[8];
    int *row = buf + t * JLD;   // this lane's block row
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = row[k];
    jpeg_fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = d[k];
    __syncthreads();

    // this lane's block column: forward column pass, quantise, dequantise, inverse column pass
    const int b = t >> 3, c = t & 7;
    int *col = buf + b * 8 * JLD + c;
    const int *tab = qt + (b >= 16 ? 64 : 0) + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = col[k * JLD];
    jpeg_fdct8<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int tq = tab[k * 8];
        const int m = (int)((unsigned)(abs(d[k]) + 4 * tq) / (unsigned)(8 * tq)) * tq;
        d[k] = d[k] < 0 ? -m : m;
    }
    jpeg_idct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k * JLD] = d[k];
    __syncthreads();

#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = row[k];
    jpeg_idct8<false>(d);
    uint2 v;
    v.x = jpeg_limit(d[0]) | (jpeg_limit(d[1]) << 8) | (jpeg_limit(d[2]) << 16) | (jpeg_limit(d[3]) << 24);
    v.y = jpeg_limit(d[4]) | (jpeg_limit(d[5]) << 8) | (jpeg_limit(d[6]) << 16) | (jpeg_limit(d[7]) << 24);
    // every plane offset below is a multiple of 8: Wp of 64, Hp of 16, block columns of 8
    unsigned char *planes = ws + (long)blockIdx.z * jpeg_image_bytes(A.Hp, A.Wp);
    const int r = t & 7;
    unsigned char *dst;
    if (b < 16) {
        dst = planes + (long)(Y0 + (b >> 3) * 8 + r) * A.Wp + X0 + (b & 7) * 8;
    } else {
        const int Hc = A.Hp / 2, Wc = A.Wp / 2, cb = b - 16;
        dst = planes + (long)A.Hp * A.Wp + (long)(cb >> 2) * Hc * Wc + (long)(Y0 / 2 + r) * Wc + X0 / 2 + (cb & 3) * 8;
    }
    *reinterpret_cast<uint2 *>(dst) = v;
}

__device__ __forceinline__ unsigned char jpeg_clamp(int v) { return (unsigned char)min(max(v, 0), 255); }

// grid (blocks of 256 pixels along w, blocks of 4 rows, n); block (JBW, JBH)
__global__ void __launch_bounds__(JBW * JBH)
k_jpeg_pixels(JpegArgs A, const unsigned char *__restrict__ ws, unsigned char *__restrict__ out) {
    const int x0 = (blockIdx.x * JBW + threadIdx.x) * 4, y = blockIdx.y * JBH + threadIdx.y;
    if (x0 >= A.w || y >= A.h) return;
    const unsigned char *planes = ws + (long)blockIdx.z * jpeg_image_bytes(A.Hp, A.Wp);
    const int Hc = A.Hp / 2, Wc = A.Wp / 2;
    const unsigned char *pcb = planes + (long)A.Hp * A.Wp, *pcr = pcb + (long)Hc * Wc;
    const unsigned yy = *reinterpret_cast<const unsigned *>(planes + (long)y * A.Wp + x0);
    const int cy = y >> 1, cx = x0 >> 1;
    int cb[4], cr[4];   // the upsampled chroma of the four pixels, - 128
    if (A.cw > 2) {
        const int ny = min(max(cy + ((y & 1) ? 1 : -1), 0), A.ch - 1);
        int sb[4], sr[4];   // 3 this + neighbour row at chroma columns cx - 1 .. cx + 2, clamped
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xc = min(max(cx - 1 + k, 0), A.cw - 1);
            sb[k] = 3 * pcb[(long)cy * Wc + xc] + pcb[(long)ny * Wc + xc];
            sr[k] = 3 * pcr[(long)cy * Wc + xc] + pcr[(long)ny * Wc + xc];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 1 + (j >> 1), o = (j & 1) ? i + 1 : i - 1, rnd = (j & 1) ? 7 : 8;
            cb[j] = ((3 * sb[i] + sb[o] + rnd) >> 4) - 128;
            cr[j] = ((3 * sr[i] + sr[o] + rnd) >> 4) - 128;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xc = min(cx + (j >> 1), A.cw - 1);
            cb[j] = pcb[(long)cy * Wc + xc] - 128;
            cr[j] = pcr[(long)cy * Wc + xc] - 128;
        }
    }
    unsigned char px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = (yy >> (8 * j)) & 255;
        px[3 * j] = jpeg_clamp(l + ((JFIX(1.402) * cr[j] + 32768) >> 16));
        px[3 * j + 1] = jpeg_clamp(l + ((-JFIX(.34414) * cb[j] + 32768 - JFIX(.71414) * cr[j]) >> 16));
        px[3 * j + 2] = jpeg_clamp(l + ((JFIX(1.772) * cb[j] + 32768) >> 16));
    }
    unsigned char *dst = out + (((long)blockIdx.z * A.h + y) * A.w + x0) * 3;
    const int m = min(4, A.w - x0);
    if (m == 4 && (((uintptr_t)dst) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<unsigned *>(dst)[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) |
                                                   ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * m; ++k) dst[k] = px[k];
    }
}

static int jpeg_shape(const char *name, int n, int h, int w, JpegArgs &A) {
    DG_ARG(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= (1 << 16) && w <= (1 << 16),
           "%s: bad shape: n %d, %dx%d", name, n, h, w);
    A.h = h; A.w = w;
    A.ch = (h + 1) / 2; A.cw = (w + 1) / 2;
    A.Hp = (h + JSH - 1) / JSH * JSH;
    A.Wp = (w + JSW - 1) / JSW * JSW;
    return DG_OK;
}

}  // namespace dg

int dg_jpeg_ws_bytes(int n, int h, int w, size_t *bytes) {
    dg::JpegArgs A;
    DG_ARG(bytes, "jpeg_ws_bytes: NULL result");
    if (int rc = dg::jpeg_shape("jpeg_ws_bytes", n, h, w, A)) return rc;
    *bytes = (size_t)n * (size_t)dg::jpeg_image_bytes(A.Hp, A.Wp);
    return DG_OK;
}

int dg_jpeg_roundtrip_u8(int n, int h, int w, const unsigned char *in, unsigned char *out, const unsigned char *qtab,
                         void *ws, size_t ws_bytes, dg_stream_t stream) {
    using namespace dg;
    JpegArgs A;
    if (int rc = jpeg_shape("jpeg_roundtrip_u8", n, h, w, A)) return rc;
    DG_ARG(qtab, "jpeg_roundtrip_u8: NULL quantisation tables");
    JpegTables Q;
    for (int i = 0; i < 128; ++i) {
        DG_ARG(qtab[i] >= 1, "jpeg_roundtrip_u8: quantisation table entry %d is 0", i);
        Q.t[i] = qtab[i];
    }
    if (n == 0) return DG_OK;
    DG_ARG(in && out && ws, "jpeg_roundtrip_u8: NULL tensor");
    const size_t need = (size_t)n * (size_t)jpeg_image_bytes(A.Hp, A.Wp);
    DG_ARG(ws_bytes >= need, "jpeg_roundtrip_u8: workspace of %zu bytes, %zu needed", ws_bytes, need);
    DG_ARG((((uintptr_t)ws) & 7) == 0, "jpeg_roundtrip_u8: the workspace must be 8-byte aligned");
    hipLaunchKernelGGL(k_jpeg_blocks, dim3(A.Wp / JSW, A.Hp / JSH, n), dim3(JT), 0, (hipStream_t)stream, A, Q, in,
                       (unsigned char *)ws);
    DG_LAUNCHED("jpeg_roundtrip_u8 (blocks)");
    hipLaunchKernelGGL(k_jpeg_pixels, dim3(dg_cdiv(dg_cdiv(w, 4), JBW), dg_cdiv(h, JBH), n), dim3(JBW, JBH), 0,
                       (hipStream_t)stream, A, (const unsigned char *)ws, out);
    DG_LAUNCHED("jpeg_roundtrip_u8 (pixels)");
    return DG_OK;
}
