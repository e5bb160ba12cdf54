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
// writes `out`, so the two may be one buffer.  The first kernel's front half, up to the quantised
// levels, is jpeg_front.h's, which the encoder (jpeg_enc.hip) shares; the inverse DCT, the range
// limit and the second kernel's launch are jpeg_back.h's, which the decoder (jpeg_dec.hip) shares.
#include "jpeg_back.h"

namespace dg {

constexpr int JBW = 64, JBH = 4;    // k_jpeg_pixels: a thread block covers 256 x 4 pixels

// grid (strips along w, strips along h, n)
__global__ void __launch_bounds__(JT)
k_jpeg_blocks(JpegArgs A, JpegTables Q, const unsigned char *__restrict__ in, unsigned char *__restrict__ ws) {
    __shared__ int buf[JT * JLD];   // block row R = block * 8 + row at R * JLD; blocks: 16 Y (2 x 8), 4 Cb, 4 Cr
    __shared__ int qt[128];
    const int t = threadIdx.x;
    const int X0 = blockIdx.x * JSW, Y0 = blockIdx.y * JSH;
    const unsigned char *img = in + (long)blockIdx.z * A.h * A.w * 3;
    int d[8], tq[8];
    jpeg_front(A, Q, img, X0, Y0, buf, qt, d, tq);

    // this lane's block column: dequantise, inverse column pass
    int *row = buf + t * JLD;   // this lane's block row
    const int b = t >> 3, c = t & 7;
    int *col = buf + b * 8 * JLD + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] *= tq[k];
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

int jpeg_launch_pixels(const char *name, const JpegArgs &A, int n, const unsigned char *ws, unsigned char *out,
                       hipStream_t stream) {
    hipLaunchKernelGGL(k_jpeg_pixels, dim3(dg_cdiv(dg_cdiv(A.w, 4), JBW), dg_cdiv(A.h, JBH), n), dim3(JBW, JBH), 0,
                       stream, A, ws, out);
    DG_LAUNCHED(name);
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
    return jpeg_launch_pixels("jpeg_roundtrip_u8 (pixels)", A, n, (const unsigned char *)ws, out, (hipStream_t)stream);
}
