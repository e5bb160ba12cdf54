// JPEG artifact removal by shift-averaged re-application (include/dgan.h "JPEG artifact removal";
// the definition and its numpy reference: dgan/filters.py dejpeg_ref).  The frame is shifted by each
// of the 64 offsets (dy, dx) of the 8 x 8 block grid (rows and columns replicated at the top and the
// left), put through the 4:2:0 round trip of dgan/jpeg.py, shifted back, and the 64 results are
// averaged.  One launch, int32 throughout, no floating point, no atomics, no workspace.
//
//   k_dejpeg   a workgroup of 256 threads owns a 64 x 64 tile of output pixels and keeps its 16
//              pixels' three sums in registers over the loop of the 64 shifts.
//     staged once per tile, every coordinate clamped into the image (which is what the shifted
//     frame's replication amounts to in the original frame's coordinates):
//       sY   luma of the tile and 7 pixels before / after it, a byte each: the block grid of shift
//            (dy, dx) starts at the tile's origin - (dy, dx)
//       sC   the four downsampling phases (dy & 1, dx & 1): the 2 x 2 SUMS of Cb and Cr (16 bits each
//            in a dword) of the cells 2k - phase, 48 x 48 cells from 8 before the tile's first.  The
//            bias of the mean follows the parity of the shifted column and is added when a block is
//            read; the row clamp ceil((h + dy) / 2) - 1 depends on the phase alone and is staged.
//            A phase serves its 16 block offsets (dy >> 1, dx >> 1).
//     per shift:
//       blocks  a lane per block row, eight neighbouring lanes per block, as the round trip's strip
//               kernel: 8 x 8 or 9 x 9 luma blocks and 5 x 5 or 6 x 6 blocks of each chroma plane
//               (the triangle filter's neighbour above / left of the tile needs a block of its own
//               when the chroma offset is 0).  Row pass, transposition through the eight lanes' rows
//               in LDS at the odd stride JLD, column pass, quantiser, dequantiser, inverse column
//               pass, transposition back, inverse row pass, range limit; the decoded bytes go to
//               dY / dC.  The eight lanes of a block sit in one wave, so the two transpositions need
//               no workgroup barrier, only the wave's own program order.
//               (|c| + 4 t) / (8 t) is one v_mul_hi_u32 with M = floor(2^32 / 8t) + 1 prepared per
//               workgroup: exact for (|c| + 4 t) * 8 t < 2^32, and |c| + 4 t < 2^16, 8 t < 2^11.
//       pixels  every thread upsamples the chroma of its 16 pixels with the shift's own clamps
//               (ch = ceil((h + dy) / 2), cw = ceil((w + dx) / 2), replication when cw <= 2),
//               converts, clamps and adds into its sums.
//     two workgroup barriers per shift; (sum + 32) >> 6 is stored once.
#include "jpeg_back.h"

namespace dg {

constexpr int DJT = 64;                  // the tile: 64 x 64 output pixels
constexpr int DJN = 256;                 // threads of a workgroup
constexpr int DJPX = DJT * DJT / DJN;    // pixels of a thread: one column, every fourth row
constexpr int DJYW = DJT + 14;           // staged luma rows / columns: 7 before the tile, 7 after
constexpr int DJYS = 80;                 // bytes of a staged luma row
constexpr int DJCK = DJT / 2 + 16;       // phase cells / decoded chroma samples per axis: six blocks
constexpr int DJDY = DJT + 8;            // decoded luma rows / columns: nine blocks
static_assert(DJN % 64 == 0 && DJT % 16 == 0 && DJDY % 8 == 0 && DJCK % 8 == 0, "blocks of eight lanes, aligned rows");

// orders the LDS accesses of one wave's lanes: the hardware runs a wave's LDS instructions in
// order, this keeps the compiler from moving them across
__device__ __forceinline__ void dejpeg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int dejpeg_clamp(int v, int hi) { return min(max(v, 0), hi); }

// grid (tiles along w, tiles along h, n)
__global__ void __launch_bounds__(DJN)
k_dejpeg(int h, int w, JpegTables Q, const unsigned char *__restrict__ in, unsigned char *__restrict__ out) {
    __shared__ unsigned sC[4 * DJCK * DJCK];                      // phase sums: Cb | Cr << 16
    __shared__ int buf[DJN * JLD];                                // a block row per lane
    __shared__ int qt[128];
    __shared__ unsigned qm[128];                                  // floor(2^32 / 8t) + 1
    __shared__ __attribute__((aligned(8))) unsigned char dY[DJDY * DJDY];      // decoded luma
    __shared__ __attribute__((aligned(8))) unsigned char dC[2 * DJCK * DJCK];  // decoded Cb, Cr
    __shared__ unsigned char sY[DJYW * DJYS];

    const int t = threadIdx.x;
    const int X0 = blockIdx.x * DJT, Y0 = blockIdx.y * DJT;
    const unsigned char *img = in + (long)blockIdx.z * h * w * 3;

    if (t < 128) {
        qt[t] = Q.t[t];
        qm[t] = 0xFFFFFFFFu / (8u * Q.t[t]) + 1u;
    }
    for (int i = t; i < DJYW * DJYW; i += DJN) {
        const int r = i / DJYW, c = i - r * DJYW;
        const int gy = dejpeg_clamp(Y0 - 7 + r, h - 1), gx = dejpeg_clamp(X0 - 7 + c, w - 1);
        sY[r * DJYS + c] = (unsigned char)jpeg_ycc(img + ((long)gy * w + gx) * 3).y;
    }
    for (int i = t; i < 4 * DJCK * DJCK; i += DJN) {
        const int ph = i / (DJCK * DJCK), j = i - ph * (DJCK * DJCK);
        const int r = j / DJCK, c = j - r * DJCK;
        const int py = ph >> 1, px = ph & 1;
        const int ky = min(Y0 / 2 - 8 + r, ((h + py + 1) >> 1) - 1), kx = X0 / 2 - 8 + c;
        const int r0 = dejpeg_clamp(2 * ky - py, h - 1), r1 = dejpeg_clamp(2 * ky - py + 1, h - 1);
        const int c0 = dejpeg_clamp(2 * kx - px, w - 1), c1 = dejpeg_clamp(2 * kx - px + 1, w - 1);
        const JpegYCC p00 = jpeg_ycc(img + ((long)r0 * w + c0) * 3), p01 = jpeg_ycc(img + ((long)r0 * w + c1) * 3);
        const JpegYCC p10 = jpeg_ycc(img + ((long)r1 * w + c0) * 3), p11 = jpeg_ycc(img + ((long)r1 * w + c1) * 3);
        sC[i] = (unsigned)(p00.cb + p01.cb + p10.cb + p11.cb) | ((unsigned)(p00.cr + p01.cr + p10.cr + p11.cr) << 16);
    }
    __syncthreads();

    int acc[DJPX][3];
#pragma unroll
    for (int i = 0; i < DJPX; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0;
    const int lx = t & (DJT - 1), ly0 = t / DJT;   // this thread's pixels: column lx, rows ly0 + (DJN / DJT) i
    const int x = X0 + lx;
    int *row = buf + t * JLD;                      // this lane's block row
    const int lane8 = t & 7;
    int *col = buf + (t & ~7) * JLD + lane8;       // this lane's block column

#pragma unroll 1
    for (int s = 0; s < 64; ++s) {
        const int dy = s >> 3, dx = s & 7, oy = dy >> 1, ox = dx >> 1;
        const int ph = ((dy & 1) << 1) | (dx & 1);
        const int nl = (dx ? 9 : 8) * (dy ? 9 : 8), nc = (ox ? 5 : 6) * (oy ? 5 : 6);
        const int ntask = (nl + 2 * nc) * 8;

        // ---- blocks: forward DCT, quantise, dequantise, inverse DCT ----
#pragma unroll 1
        for (int T = t; T < ntask; T += DJN) {
            int blk = T >> 3;
            int d[8];
            const int *tab;
            const unsigned *mag;
            unsigned char *dst;
            if (blk < nl) {
                const int by = dx ? blk / 9 : blk >> 3, bx = blk - by * (dx ? 9 : 8);
                const unsigned char *src = sY + (7 - dy + 8 * by + lane8) * DJYS + 7 - dx + 8 * bx;
#pragma unroll
                for (int k = 0; k < 8; ++k) d[k] = (int)src[k] - 128;
                tab = qt;
                mag = qm;
                dst = dY + (8 * by + lane8) * DJDY + 8 * bx;
            } else {
                blk -= nl;
                const int comp = blk >= nc;
                if (comp) blk -= nc;
                const int by = ox ? blk / 5 : blk / 6, bx = blk - by * (ox ? 5 : 6);
                // the decoded plane starts at a multiple of 8 of the shifted chroma grid, eight cells
                // before the tile's first when the offset is 0; cell k of a phase = shifted cell - offset
                const unsigned *src = sC + ph * (DJCK * DJCK) + ((oy ? 8 - oy : 0) + 8 * by + lane8) * DJCK +
                                      (ox ? 8 - ox : 0) + 8 * bx;
                const int sh = comp ? 16 : 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) d[k] = (int)((((src[k] >> sh) & 0xFFFFu) + 1u + (k & 1)) >> 2) - 128;
                tab = qt + 64;
                mag = qm + 64;
                dst = dC + comp * (DJCK * DJCK) + (8 * by + lane8) * DJCK + 8 * bx;
            }
            jpeg_fdct8<true>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) row[k] = d[k];
            dejpeg_wave_sync();
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = col[k * JLD];
            jpeg_fdct8<false>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int tq = tab[k * 8 + lane8];
                const int m = (int)__umulhi((unsigned)(abs(d[k]) + 4 * tq), mag[k * 8 + lane8]);
                d[k] = (d[k] < 0 ? -m : m) * tq;
            }
            jpeg_idct8<true>(d);
            dejpeg_wave_sync();
#pragma unroll
            for (int k = 0; k < 8; ++k) col[k * JLD] = d[k];
            dejpeg_wave_sync();
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = row[k];
            jpeg_idct8<false>(d);
            uint2 v;
            v.x = jpeg_limit(d[0]) | (jpeg_limit(d[1]) << 8) | (jpeg_limit(d[2]) << 16) | (jpeg_limit(d[3]) << 24);
            v.y = jpeg_limit(d[4]) | (jpeg_limit(d[5]) << 8) | (jpeg_limit(d[6]) << 16) | (jpeg_limit(d[7]) << 24);
            *reinterpret_cast<uint2 *>(dst) = v;
            dejpeg_wave_sync();
        }
        __syncthreads();

        // ---- pixels: upsample, convert, clamp, accumulate ----
        if (x < w) {
            const int chs = (h + dy + 1) >> 1, cws = (w + dx + 1) >> 1;   // the shifted frame's chroma plane
            const int cy0 = Y0 / 2 - (oy ? 0 : 8), cx0 = X0 / 2 - (ox ? 0 : 8);
            const int xs = x + dx, cx = xs >> 1;
            const int xo = (xs & 1) ? min(cx + 1, cws - 1) : max(cx - 1, 0);
            const int rnd = (xs & 1) ? 7 : 8;
            const bool fancy = cws > 2;
            const unsigned char *pb = dC, *pr = dC + DJCK * DJCK;
#pragma unroll
            for (int i = 0; i < DJPX; ++i) {
                const int ly = ly0 + (DJN / DJT) * i;
                if (Y0 + ly < h) {
                    const int ys = Y0 + ly + dy, cy = ys >> 1;
                    const int l = dY[(ly + dy) * DJDY + lx + dx];
                    const int i00 = (cy - cy0) * DJCK + cx - cx0;
                    int cb, cr;
                    if (fancy) {
                        const int ny = dejpeg_clamp(cy + ((ys & 1) ? 1 : -1), chs - 1);
                        const int i01 = (cy - cy0) * DJCK + xo - cx0;
                        const int i10 = (ny - cy0) * DJCK + cx - cx0, i11 = (ny - cy0) * DJCK + xo - cx0;
                        cb = ((3 * (3 * pb[i00] + pb[i10]) + 3 * pb[i01] + pb[i11] + rnd) >> 4) - 128;
                        cr = ((3 * (3 * pr[i00] + pr[i10]) + 3 * pr[i01] + pr[i11] + rnd) >> 4) - 128;
                    } else {
                        cb = pb[i00] - 128;
                        cr = pr[i00] - 128;
                    }
                    acc[i][0] += dejpeg_clamp(l + ((JFIX(1.402) * cr + 32768) >> 16), 255);
                    acc[i][1] += dejpeg_clamp(l + ((-JFIX(.34414) * cb + 32768 - JFIX(.71414) * cr) >> 16), 255);
                    acc[i][2] += dejpeg_clamp(l + ((JFIX(1.772) * cb + 32768) >> 16), 255);
                }
            }
        }
        __syncthreads();
    }

    if (x < w) {
        unsigned char *o = out + (long)blockIdx.z * h * w * 3;
#pragma unroll
        for (int i = 0; i < DJPX; ++i) {
            const int y = Y0 + ly0 + (DJN / DJT) * i;
            if (y < h) {
                unsigned char *p = o + ((long)y * w + x) * 3;
                p[0] = (unsigned char)((acc[i][0] + 32) >> 6);
                p[1] = (unsigned char)((acc[i][1] + 32) >> 6);
                p[2] = (unsigned char)((acc[i][2] + 32) >> 6);
            }
        }
    }
}

}  // namespace dg

int dg_dejpeg(int n, int h, int w, const unsigned char *in, unsigned char *out, const unsigned char *qtab,
              dg_stream_t stream) {
    using namespace dg;
    DG_ARG(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= (1 << 16) && w <= (1 << 16),
           "dejpeg: bad shape: n %d, %dx%d", n, h, w);
    DG_ARG(qtab, "dejpeg: NULL quantisation tables");
    JpegTables Q;
    for (int i = 0; i < 128; ++i) {
        DG_ARG(qtab[i] >= 1, "dejpeg: quantisation table entry %d is 0", i);
        Q.t[i] = qtab[i];
    }
    if (n == 0) return DG_OK;
    DG_ARG(in && out, "dejpeg: NULL tensor");
    DG_ARG(in != out, "dejpeg: the output must not be the input");
    hipLaunchKernelGGL(k_dejpeg, dim3(dg_cdiv(w, DJT), dg_cdiv(h, DJT), n), dim3(DJN), 0, (hipStream_t)stream, h, w, Q,
                       in, out);
    DG_LAUNCHED("dejpeg");
    return DG_OK;
}
