// The back half of libjpeg's decompressor at 4:2:0, shared by the round trip (jpeg.hip) and the
// decoder (jpeg_dec.hip): the islow inverse DCT pass, the range limit, the layout of the decoded
// uint8 planes and the launch of the pixel kernel (chroma upsampling and colour, jpeg.hip).
#pragma once
#include "jpeg_front.h"

namespace dg {

// the decoded planes of one image: Y [Hp][Wp], then Cb and Cr [Hp/2][Wp/2]
__host__ __device__ __forceinline__ long jpeg_image_bytes(int Hp, int Wp) { return (long)Hp * Wp / 2 * 3; }

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

// k_jpeg_pixels (jpeg.hip) on the planes of n images at `ws`: out[n][h][w][3]
int jpeg_launch_pixels(const char *name, const JpegArgs &A, int n, const unsigned char *ws, unsigned char *out,
                       hipStream_t stream);

}  // namespace dg
