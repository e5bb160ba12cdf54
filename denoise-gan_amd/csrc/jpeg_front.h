// The front half of libjpeg's compressor at 4:2:0, shared by the round trip (jpeg.hip) and the
// encoder (jpeg_enc.hip): colour conversion, chroma downsampling, the islow forward DCT and
// quantisation of one 64x16 strip of four MCUs, in the integer arithmetic of dgan/jpeg.py.
#pragma once
#include "common.h"

namespace dg {

constexpr int JT = 192;             // threads of a strip kernel: one per block row, 24 blocks of 8
constexpr int JSW = 64, JSH = 16;   // luma pixels of a strip: four MCUs side by side
constexpr int JLD = 9;              // ints per block row in LDS: odd, so that the 32 lanes of a row
                                    // pass (stride JLD) and of a column pass (8 blocks x 8 columns)
                                    // each hit 32 different banks
static_assert(JT == (JSW / 8) * (JSH / 8) * 8 * 3 / 2, "one lane per block row of the strip");

struct JpegTables {
    unsigned char t[128];   // luminance [64], chrominance [64], row-major
};

struct JpegArgs {
    int h, w, ch, cw;   // image, chroma plane
    int Hp, Wp;         // luma plane of the workspace: h, w rounded up to the strip
};

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

// The strip at (X0, Y0) of `img` [h][w][3] through colour conversion, downsampling, both forward
// DCT passes and quantisation.  Called by all JT threads of a block with buf[JT * JLD] and qt[128]
// in LDS: block row R = block * 8 + row sits at R * JLD; blocks: 16 Y (2 x 8), 4 Cb, 4 Cr.  On
// return lane t holds column t & 7 of block t >> 3: d[k] the signed quantised level of row k, tq[k]
// its table entry; buf holds the row pass's output and every lane has read its column.
__device__ __forceinline__ void jpeg_front(const JpegArgs &A, const JpegTables &Q, const unsigned char *img, int X0,
                                           int Y0, int *buf, int *qt, int d[8], int tq[8]) {
    const int t = threadIdx.x;
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

    int *row = buf + t * JLD;   // this lane's block row
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = row[k];
    jpeg_fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = d[k];
    __syncthreads();

    // this lane's block column: forward column pass, quantise
    const int b = t >> 3, c = t & 7;
    const int *col = buf + b * 8 * JLD + c;
    const int *tab = qt + (b >= 16 ? 64 : 0) + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = col[k * JLD];
    jpeg_fdct8<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        tq[k] = tab[k * 8];
        const int m = (int)((unsigned)(abs(d[k]) + 4 * tq[k]) / (unsigned)(8 * tq[k]));
        d[k] = d[k] < 0 ? -m : m;
    }
}

static inline int jpeg_shape(const char *name, int n, int h, int w, JpegArgs &A) {
    DG_ARG(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= (1 << 16) && w <= (1 << 16),
           "%s: bad shape: n %d, %dx%d", name, n, h, w);
    A.h = h; A.w = w;
    A.ch = (h + 1) / 2; A.cw = (w + 1) / 2;
    A.Hp = (h + JSH - 1) / JSH * JSH;
    A.Wp = (w + JSW - 1) / JSW * JSW;
    return DG_OK;
}

}  // namespace dg
