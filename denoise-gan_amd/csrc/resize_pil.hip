// Pillow's Image.resize on the device (include/dgan.h "Image resize, Pillow's"; the coefficient
// tables and the integer reference: dgan/resize.py pil_coeffs, resize_pil_ref).  Integers only, one
// launch for both passes, no intermediate in HBM: a block owns a tile of th x tw output pixels of one
// image.  Phase 1 runs the horizontal pass over the input rows the tile's vertical taps touch and
// leaves the clipped uint8 intermediate [rows][tw * C] in LDS; phase 2 walks each output byte's
// vertical taps down LDS.  The tile is chosen on the host (pil_tile) so that the intermediate and
// the tile's coefficients fit PIL_LDS; the kernel clamps every table entry into what it was given,
// so tables of another origin give other pixels, never an access outside the image or the LDS.
#include "common.h"

namespace dg {

constexpr int PIL_T = 256;               // threads per block
constexpr int PIL_TH = 16, PIL_TW = 64;  // the largest output tile
constexpr int PIL_LDS = 64 * 1024;       // bytes of LDS a block may use
constexpr int PIL_KX = 16 * 1024;        // of which the x coefficients take at most this, while tw > 1
constexpr int PIL_BITS = 22;             // fraction bits of a coefficient

struct PilArgs {
    int hi, wi, ho, wo, ksx, ksy;
    int th, tw;   // the output tile
    int rows;     // intermediate rows the LDS holds
    int s4;       // their stride in dwords, odd
    int tiles_x;
};

// dwords of LDS of a tile: first / count of both axes, both coefficient slices, the intermediate
__host__ __device__ __forceinline__ long pil_lds_dwords(const PilArgs &A) {
    return 2L * A.tw + 2L * A.th + (long)A.tw * A.ksx + (long)A.th * A.ksy + (long)A.rows * A.s4;
}

// Rows a tile of th outputs touches: consecutive centres lie hi / ho apart, so the first taps of
// the tile's top and bottom rows lie at most ceil((th - 1) hi / ho) apart, and a row has at most
// ksy taps.
static int pil_rows(int hi, int ho, int ksy, int th) {
    const long r = ((long)(th - 1) * hi + ho - 1) / ho + ksy;
    return (int)(r < hi ? r : hi);
}

// The tile of one problem: the smallest powers of two covering the output, at most PIL_TH x PIL_TW;
// tw halves while the x coefficients overflow their share, then th halves, then tw again, until the
// block fits.  false: not even one output pixel per block fits.
static bool pil_tile(int hi, int wi, int C, int ho, int wo, int ksx, int ksy, PilArgs &A) {
    A.hi = hi; A.wi = wi; A.ho = ho; A.wo = wo; A.ksx = ksx; A.ksy = ksy;
    A.th = PIL_TH; A.tw = PIL_TW;
    while (A.th / 2 >= ho) A.th /= 2;
    while (A.tw / 2 >= wo) A.tw /= 2;
    while (A.tw > 1 && (long)A.tw * ksx * 4 > PIL_KX) A.tw /= 2;
    for (;;) {
        A.rows = pil_rows(hi, ho, ksy, A.th);
        A.s4 = ((A.tw * C + 3) / 4) | 1;
        A.tiles_x = (int)dg_cdiv(wo, A.tw);
        if (pil_lds_dwords(A) * 4 <= PIL_LDS) return true;
        if (A.th > 1) A.th /= 2;
        else if (A.tw > 1) A.tw /= 2;
        else return false;
    }
}

__device__ __forceinline__ int pil_clip8(int acc) { return min(max(acc >> PIL_BITS, 0), 255); }

// grid (tiles along w * tiles along h, 1, n); dynamic LDS of pil_lds_dwords
template <int C>
__global__ void __launch_bounds__(PIL_T)
k_resize_pil(PilArgs A, const unsigned char *__restrict__ in, unsigned char *__restrict__ out,
             const int *__restrict__ fx, const int *__restrict__ cx, const int *__restrict__ kx,
             const int *__restrict__ fy, const int *__restrict__ cy, const int *__restrict__ ky) {
    extern __shared__ int pil_lds[];
    int *fxs = pil_lds, *cxs = fxs + A.tw, *fys = cxs + A.tw, *cys = fys + A.th;
    int *kxs = cys + A.th, *kys = kxs + A.tw * A.ksx;
    unsigned *mid = reinterpret_cast<unsigned *>(kys + A.th * A.ksy);
    const int t = threadIdx.x;
    const int by = blockIdx.x / A.tiles_x, bx = blockIdx.x - by * A.tiles_x;
    const int oy0 = by * A.th, ox0 = bx * A.tw;
    const int th = min(A.th, A.ho - oy0), tw = min(A.tw, A.wo - ox0);

    // the tile's slice of the six tables, first and count clamped into the image
    for (int i = t; i < tw; i += PIL_T) {
        const int f = min(max(fx[ox0 + i], 0), A.wi - 1);
        fxs[i] = f;
        cxs[i] = min(max(cx[ox0 + i], 0), min(A.ksx, A.wi - f));
    }
    for (int i = t; i < th; i += PIL_T) {
        const int f = min(max(fy[oy0 + i], 0), A.hi - 1);
        fys[i] = f;
        cys[i] = min(max(cy[oy0 + i], 0), min(A.ksy, A.hi - f));
    }
    for (int i = t; i < tw * A.ksx; i += PIL_T) kxs[i] = kx[(long)ox0 * A.ksx + i];
    for (int i = t; i < th * A.ksy; i += PIL_T) kys[i] = ky[(long)oy0 * A.ksy + i];
    __syncthreads();

    // the input rows of the tile: y0 .. y0 + nrows - 1, never more than the LDS holds
    int y0 = A.hi, y1 = 0;
    for (int r = 0; r < th; ++r) {
        y0 = min(y0, fys[r]);
        y1 = max(y1, fys[r] + cys[r]);
    }
    const int nrows = min(y1 - y0, A.rows);
    const int twc = tw * C;
    const unsigned char *img = in + (long)blockIdx.z * A.hi * A.wi * C;

    // Phase 1, horizontal: a lane per byte of an intermediate row, so neighbouring lanes read
    // neighbouring (for an upscale, the same) bytes of the input row.  The tap loop ends at the
    // lane's own count: a wave runs to the largest count of its outputs, not to ksx.
    unsigned char *midb = reinterpret_cast<unsigned char *>(mid);
    for (int g = t; g < nrows * twc; g += PIL_T) {
        const int r = g / twc, q = g - r * twc;
        const int o = q / C, c = q - o * C;
        const unsigned char *p = img + ((long)(y0 + r) * A.wi + fxs[o]) * C + c;
        const int *k = kxs + o * A.ksx;
        const int cnt = cxs[o];
        int acc = 1 << (PIL_BITS - 1);
        for (int j = 0; j < cnt; ++j) acc = __mul24(k[j], (int)p[j * C]) + acc;
        midb[(r * A.s4) * 4 + q] = (unsigned char)pil_clip8(acc);
    }
    __syncthreads();

    // Phase 2, vertical: a lane owns four consecutive bytes of an output row segment and walks its
    // taps down LDS, one dword per tap (row stride odd in dwords: lanes of different output rows
    // start in different banks), accumulates in int32 and stores them packed.
    const int ng = (twc + 3) >> 2;
    unsigned char *orow = out + (((long)blockIdx.z * A.ho + oy0) * A.wo + ox0) * C;
    const long ostride = (long)A.wo * C;
    for (int g = t; g < th * ng; g += PIL_T) {
        const int r = g / ng, g4 = g - r * ng;
        const int m = min(4, twc - g4 * 4);
        const int f = fys[r] - y0;
        const int cnt = min(cys[r], nrows - f);
        const unsigned *s = mid + f * A.s4 + g4;
        const int *k = kys + r * A.ksy;
        int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int j = 0; j < cnt; ++j) {
            const unsigned v = s[j * A.s4];
            const int kk = k[j];
            a0 = __mul24(kk, (int)(v & 255u)) + a0;
            a1 = __mul24(kk, (int)((v >> 8) & 255u)) + a1;
            a2 = __mul24(kk, (int)((v >> 16) & 255u)) + a2;
            a3 = __mul24(kk, (int)(v >> 24)) + a3;
        }
        const unsigned b0 = pil_clip8(a0), b1 = pil_clip8(a1), b2 = pil_clip8(a2), b3 = pil_clip8(a3);
        unsigned char *p = orow + r * ostride + g4 * 4;
        if (m == 4 && (((uintptr_t)p) & 3) == 0) {
            *reinterpret_cast<unsigned *>(p) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        } else {
            const unsigned b[4] = {b0, b1, b2, b3};
            for (int j = 0; j < m; ++j) p[j] = (unsigned char)b[j];
        }
    }
}

static int pil_check(const char *name, int n, int hi, int wi, int C, int ho, int wo, int ksx, int ksy) {
    const int lim = 1 << 20;   // (as dg_resize_u8: element offsets stay far inside 64 bits)
    DG_ARG(n >= 0 && n <= 65535 && hi >= 1 && wi >= 1 && ho >= 1 && wo >= 1 && hi <= lim && wi <= lim && ho <= lim &&
               wo <= lim && (long)hi * wi <= (1L << 34) && (long)ho * wo <= (1L << 34),
           "%s: bad shape: n %d, %dx%d -> %dx%d", name, n, hi, wi, ho, wo);
    DG_ARG(C == 1 || C == 3, "%s: C must be 1 or 3, got %d", name, C);
    DG_ARG(ksx >= 1 && ksy >= 1 && ksx <= 4 * lim && ksy <= 4 * lim, "%s: bad ksize: %d, %d", name, ksx, ksy);
    return DG_OK;
}

}  // namespace dg

int dg_resize_pil_tile(int hi, int wi, int C, int ho, int wo, int ksx, int ksy, int *th, int *tw, size_t *lds_bytes) {
    if (int rc = dg::pil_check("resize_pil_tile", 1, hi, wi, C, ho, wo, ksx, ksy)) return rc;
    DG_ARG(th && tw && lds_bytes, "resize_pil_tile: NULL result");
    dg::PilArgs A;
    DG_ARG(dg::pil_tile(hi, wi, C, ho, wo, ksx, ksy, A),
           "resize_pil_tile: %dx%d -> %dx%d with %d x %d taps: one output pixel's rows and coefficients exceed the "
           "%d bytes of LDS of a block", hi, wi, ho, wo, ksx, ksy, dg::PIL_LDS);
    *th = A.th;
    *tw = A.tw;
    *lds_bytes = (size_t)dg::pil_lds_dwords(A) * 4;
    return DG_OK;
}

int dg_resize_pil_u8(int n, int hi, int wi, int C, int ho, int wo, const unsigned char *in, unsigned char *out,
                     const int *fx, const int *cx, const int *kx, int ksx, const int *fy, const int *cy, const int *ky,
                     int ksy, dg_stream_t stream) {
    const char *name = "resize_pil_u8";
    if (int rc = dg::pil_check(name, n, hi, wi, C, ho, wo, ksx, ksy)) return rc;
    if (n == 0) return DG_OK;
    DG_ARG(in && out && fx && cx && kx && fy && cy && ky, "%s: NULL tensor", name);
    DG_ARG(in != out, "%s: in and out are the same buffer", name);
    DG_ARG(((((uintptr_t)fx) | ((uintptr_t)cx) | ((uintptr_t)kx) | ((uintptr_t)fy) | ((uintptr_t)cy) | ((uintptr_t)ky)) & 3) == 0,
           "%s: misaligned coefficient tables", name);
    dg::PilArgs A;
    DG_ARG(dg::pil_tile(hi, wi, C, ho, wo, ksx, ksy, A),
           "%s: %dx%d -> %dx%d with %d x %d taps: one output pixel's rows and coefficients exceed the %d bytes of LDS "
           "of a block", name, hi, wi, ho, wo, ksx, ksy, dg::PIL_LDS);
    const long tiles = (long)A.tiles_x * dg_cdiv(ho, A.th);
    DG_ARG(tiles < (1L << 24), "%s: %ld tiles of %dx%d, more than a grid of 2^32 threads holds", name, tiles, A.th, A.tw);
    const size_t lds = (size_t)dg::pil_lds_dwords(A) * 4;
    const dim3 grid((unsigned)tiles, 1, n);
    if (C == 3)
        hipLaunchKernelGGL(dg::k_resize_pil<3>, grid, dim3(dg::PIL_T), lds, (hipStream_t)stream, A, in, out, fx, cx, kx, fy,
                           cy, ky);
    else
        hipLaunchKernelGGL(dg::k_resize_pil<1>, grid, dim3(dg::PIL_T), lds, (hipStream_t)stream, A, in, out, fx, cx, kx, fy,
                           cy, ky);
    DG_LAUNCHED(name);
    return DG_OK;
}
