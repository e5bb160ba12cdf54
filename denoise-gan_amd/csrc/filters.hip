// Classical denoisers on dense uint8 RGB frames (include/dgan.h "Classical filters"; the integer
// definitions and their numpy references: dgan/filters.py).  Integer arithmetic only, no atomics:
// a result depends on the image alone, never on the order the tiles ran in.
//
//   k_median3  the frame as h rows of 3 w bytes, where a byte's horizontal neighbours sit 3 bytes
//              away.  A thread owns 4 consecutive bytes of MROWS rows and walks down them with
//              three rows of 10 bytes in registers, so a row is loaded once for the three output
//              rows that read it.  Every byte column of the three rows is sorted by three
//              exchanges; the median of 9 is then med3(max of the three lows, med3 of the three
//              middles, min of the three highs), a fixed network of min / max with no loop over
//              the values and no branch on them.  A sorted column serves the three outputs that
//              share it.
//
//   k_nlm      a workgroup of 256 threads owns a 32 x 32 output tile.  The tile and its apron of
//              r = t/2 + s/2 pixels are staged once into LDS, a pixel per dword (its bytes R G B 0
//              from the low end, reflection resolved here), beside the weight table as uint16.  For one
//              offset d the patch distance of pixel p is a t x t box sum over the per-position
//              channel-summed squared difference e_d; it is formed separably, O(t) per pixel:
//                phase 1  152 threads (t = 7) each own one row of the tile's (32+t-1)^2 extent and
//                         8 consecutive columns: 8+t-1 values of e_d, each computed once, and their
//                         horizontal running sums H in registers; H goes to LDS
//                barrier
//                phase 2  every thread owns 4 vertically adjacent pixels of one column: 4+t-1 values
//                         of H from LDS, the vertical running sum, the table lookup, and the
//                         accumulation of S and of the three weighted channel sums in registers
//              H is double-buffered, so the next offset's phase 1 writes the other buffer and ONE
//              barrier per offset is all the split needs (phase 1 of offset k+1 can only start
//              after the barrier of offset k, which every thread passes after its phase 2 of
//              offset k-1).  When the weight table is too large for two buffers beside it in
//              64 KB (h >= 39: 15816 entries) H is single and a second barrier closes the offset.
//              Lanes read and write LDS at consecutive dwords or at an odd row stride, chosen so
//              that neither phase should meet bank conflicts (from the addresses; not measured).
//              e_d as a dot product: (a - b)^2 summed = a.a + b.b - 2 a.b, and the box sums of a.a
//              are offset-independent: N, the t x t box sum of the pixels' own squares over the
//              tile and its search apron, is formed once per tile in LDS, and per offset only the
//              cross term a.b is left, one v_dot4_u32_u8 per position with the base pixel in a
//              register for the whole offset loop: D = N(p) + N(p+d) - 2 box(a.b), exact in int32.
//              (Forming e_d channel by channel instead, three subtractions and multiply-adds on
//              extracted bytes and no N, measured 1.29 - 1.33 x slower at t = 7, s = 21 and
//              1.17 - 1.18 x at t = 3, s = 7 on 1080p frames: DESIGN.md, Classical filters.)
#include "common.h"

namespace dg {

// ---------------------------------------------------------------------------------------------
// 3x3 median
// ---------------------------------------------------------------------------------------------
constexpr int MBX = 64, MBY = 4;   // thread block: 64 x 4 bytes of a row, 4 bands of rows
constexpr int MROWS = 4;           // rows a thread walks down

__device__ __forceinline__ void exchange(int &a, int &b) {
    const int lo = min(a, b);
    b = max(a, b);
    a = lo;
}

__device__ __forceinline__ int med3(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }

// grid (blocks of 256 row bytes, blocks of 16 rows, n)
__global__ void __launch_bounds__(MBX * MBY)
k_median3(int h, int w3, const unsigned char *__restrict__ in, unsigned char *__restrict__ out) {
    const int i0 = (blockIdx.x * MBX + threadIdx.x) * 4;
    const int y0 = (blockIdx.y * MBY + threadIdx.y) * MROWS;
    if (i0 >= w3 || y0 >= h) return;
    const long image = (long)blockIdx.z * h * w3;
    in += image;
    out += image;
    // byte columns i0 - 3 .. i0 + 6; a column outside the row is its output's own (edge replication)
    int col[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        int j = i0 - 3 + k;
        if (j < 0) j += 3;
        if (j >= w3) j -= 3;
        col[k] = min(j, w3 - 1);   // (columns only outputs past the row end would read)
    }
    int a[10], b[10], c[10];
    const unsigned char *ra = in + (long)max(y0 - 1, 0) * w3, *rb = in + (long)y0 * w3;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        a[k] = ra[col[k]];
        b[k] = rb[col[k]];
    }
#pragma unroll
    for (int r = 0; r < MROWS; ++r) {
        const int y = y0 + r;
        if (y >= h) break;
        const unsigned char *rc = in + (long)min(y + 1, h - 1) * w3;
        int lo[10], mid[10], hi[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            c[k] = rc[col[k]];
            lo[k] = a[k];
            mid[k] = b[k];
            hi[k] = c[k];
            exchange(lo[k], mid[k]);
            exchange(mid[k], hi[k]);
            exchange(lo[k], mid[k]);
        }
        unsigned m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            m[q] = (unsigned)med3(max(max(lo[q], lo[q + 3]), lo[q + 6]), med3(mid[q], mid[q + 3], mid[q + 6]),
                                  min(min(hi[q], hi[q + 3]), hi[q + 6]));
        unsigned char *dst = out + (long)y * w3 + i0;
        const int left = min(4, w3 - i0);
        if (left == 4 && (((uintptr_t)dst) & 3) == 0) {
            *reinterpret_cast<unsigned *>(dst) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
        } else {
            for (int q = 0; q < left; ++q) dst[q] = (unsigned char)m[q];
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            a[k] = b[k];
            b[k] = c[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// non-local means
// ---------------------------------------------------------------------------------------------
constexpr int NT = 256;               // threads of a workgroup
constexpr int NTH = 32, NTW = 32;     // output tile
constexpr int NSEG = 8;               // phase 1: extent columns per thread
constexpr int NPIX = 4;               // phase 2: pixels (rows) per thread
constexpr int NRS = 10, NRT = 3;      // largest search and template radius
constexpr int NPLD = NTW + 2 * (NRS + NRT) + 1;   // dwords per staged pixel row: odd
constexpr int NPSZ = (NTH + 2 * (NRS + NRT)) * NPLD;
constexpr int NNLD = NTW + 2 * NRS;               // dwords per row of N
constexpr int NNSZ = (NTH + 2 * NRS) * NNLD;
constexpr int NHLD = NTW + 1;                     // dwords per row of H: odd
constexpr int NHSZ = (NTH + 2 * NRT) * NHLD;
constexpr int NLDS_MAX = 64 * 1024;
static_assert(NT == NTW * (NTH / NPIX), "phase 2: one thread per column and band of NPIX rows");
static_assert((NTH + 2 * NRT) * (NTW / NSEG) <= NT, "phase 1: one thread per extent row and column segment");

// np.pad's "reflect" for any pad width (dgan/infer.py pad_index)
__device__ __forceinline__ int reflect(int v, int size) {
    if (size == 1) return 0;
    const int p = 2 * (size - 1);
    int j = v % p;
    if (j < 0) j += p;
    return j >= size ? p - j : j;
}

// grid (tiles along w, tiles along h, n); dynamic LDS: pixels, N, H x hbufs, the table
template <int T>
__global__ void __launch_bounds__(NT)
k_nlm(int h, int w, int rs, int hbufs, const unsigned short *__restrict__ table, int tlen,
      const unsigned char *__restrict__ in, unsigned char *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    constexpr int RT = T / 2, NROW = NTH + T - 1, NEV = NSEG + T - 1, NV = NPIX + T - 1;
    int *P = lds, *Nb = P + NPSZ, *H = Nb + NNSZ;
    unsigned short *tab = reinterpret_cast<unsigned short *>(H + hbufs * NHSZ);
    const int tid = threadIdx.x, r = RT + rs;
    const int X0 = blockIdx.x * NTW, Y0 = blockIdx.y * NTH;
    const long image = (long)blockIdx.z * h * w * 3;

    // the tile and its apron, reflected into the image; the table
    const int ph = NTH + 2 * r, pw = NTW + 2 * r;
    for (int i = tid; i < ph * pw; i += NT) {
        const int ly = i / pw, lx = i - ly * pw;
        const unsigned char *p = in + image + ((long)reflect(Y0 + ly - r, h) * w + reflect(X0 + lx - r, w)) * 3;
        P[ly * NPLD + lx] = (int)((unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16));
    }
    for (int i = tid; i < tlen; i += NT) tab[i] = table[i];
    __syncthreads();

    // phase 2 role: pixels (py0 + k, px), k < NPIX
    const int px = tid & (NTW - 1), py0 = (tid / NTW) * NPIX;
    // N[u][v] = the t x t box sum of the pixels' own squares from staged (u, v) on
    const int nh = NTH + 2 * rs, nw = NTW + 2 * rs;
    for (int i = tid; i < nh * nw; i += NT) {
        const int u = i / nw, v = i - u * nw;
        unsigned sum = 0;
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const unsigned q = (unsigned)P[(u + j) * NPLD + v + k];
                sum = __builtin_amdgcn_udot4(q, q, sum, false);
            }
        Nb[u * NNLD + v] = (int)sum;
    }
    __syncthreads();
    int Np[NPIX];
#pragma unroll
    for (int k = 0; k < NPIX; ++k) Np[k] = Nb[(py0 + k + rs) * NNLD + px + rs];

    // phase 1 role: extent row ey, extent columns seg * NSEG .. + NSEG - 1; the base pixels of
    // their NEV positions stay in registers for every offset
    const bool p1 = tid < NROW * (NTW / NSEG);
    const int seg = p1 ? tid / NROW : 0, ey = p1 ? tid - seg * NROW : 0;
    const int *pa = P + (ey + rs) * NPLD + seg * NSEG + rs;
    unsigned a[NEV];
#pragma unroll
    for (int j = 0; j < NEV; ++j) a[j] = (unsigned)pa[j];

    int S[NPIX], A[NPIX][3];
#pragma unroll
    for (int k = 0; k < NPIX; ++k) S[k] = A[k][0] = A[k][1] = A[k][2] = 0;

    int buf = 0;
    for (int dy = -rs; dy <= rs; ++dy) {
        for (int dx = -rs; dx <= rs; ++dx) {
            int *Hb = H + buf * NHSZ;
            if (p1) {
                const int *pb = pa + dy * NPLD + dx;
                int c[NEV];
#pragma unroll
                for (int j = 0; j < NEV; ++j) c[j] = (int)__builtin_amdgcn_udot4(a[j], (unsigned)pb[j], 0u, false);
                int run = 0;
#pragma unroll
                for (int j = 0; j < T; ++j) run += c[j];
                int *hw = Hb + ey * NHLD + seg * NSEG;
                hw[0] = run;
#pragma unroll
                for (int x = 1; x < NSEG; ++x) {
                    run += c[x + T - 1] - c[x - 1];
                    hw[x] = run;
                }
            }
            __syncthreads();   // the one barrier of an offset: H written -> H read

            const int *hr = Hb + py0 * NHLD + px;
            int v[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] = hr[j * NHLD];
            int box = 0;
#pragma unroll
            for (int j = 0; j < T; ++j) box += v[j];
            const int *pq = P + (py0 + r + dy) * NPLD + px + r + dx;
            const int *pn = Nb + (py0 + rs + dy) * NNLD + px + rs + dx;
#pragma unroll
            for (int k = 0; k < NPIX; ++k) {
                if (k) box += v[k + T - 1] - v[k - 1];
                const unsigned D = (unsigned)(Np[k] + pn[k * NNLD] - 2 * box);
                const int wgt = tab[min(D / (unsigned)(3 * T * T), (unsigned)(tlen - 1))];
                const unsigned q = (unsigned)pq[k * NPLD];
                S[k] += wgt;
                A[k][0] += wgt * (int)(q & 255);
                A[k][1] += wgt * (int)((q >> 8) & 255);
                A[k][2] += wgt * (int)(q >> 16);
            }
            if (hbufs == 2) buf ^= 1;
            else __syncthreads();   // single H: read -> the next offset's write
        }
    }

    const int x = X0 + px;
#pragma unroll
    for (int k = 0; k < NPIX; ++k) {
        const int y = Y0 + py0 + k;
        if (y < h && x < w) {
            unsigned char *dst = out + image + ((long)y * w + x) * 3;
            const unsigned s = (unsigned)S[k];   // >= W[0]: the centre offset
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = (unsigned char)(((unsigned)A[k][c] + s / 2) / s);
        }
    }
}

static int filter_shape(const char *name, int n, int h, int w) {
    DG_ARG(n >= 0 && n <= 65535 && h >= 1 && w >= 1 && h <= (1 << 16) && w <= (1 << 16),
           "%s: bad shape: n %d, %dx%d", name, n, h, w);
    return DG_OK;
}

}  // namespace dg

int dg_median3_u8(int n, int h, int w, const unsigned char *in, unsigned char *out, dg_stream_t stream) {
    using namespace dg;
    if (int rc = filter_shape("median3_u8", n, h, w)) return rc;
    if (n == 0) return DG_OK;
    DG_ARG(in && out, "median3_u8: NULL tensor");
    DG_ARG(in != out, "median3_u8: the output must not be the input");
    hipLaunchKernelGGL(k_median3, dim3(dg_cdiv(3L * w, 4 * MBX), dg_cdiv(h, MBY * MROWS), n), dim3(MBX, MBY), 0,
                       (hipStream_t)stream, h, 3 * w, in, out);
    DG_LAUNCHED("median3_u8");
    return DG_OK;
}

int dg_nlm_u8(int n, int h, int w, int t, int s, const unsigned short *table, int table_len, const unsigned char *in,
              unsigned char *out, dg_stream_t stream) {
    using namespace dg;
    const char *name = "nlm_u8";
    if (int rc = filter_shape(name, n, h, w)) return rc;
    DG_ARG(t == 3 || t == 5 || t == 7, "%s: the template must be 3, 5 or 7, got %d", name, t);
    DG_ARG(s >= 3 && s <= 2 * NRS + 1 && (s & 1), "%s: the search window must be odd in 3..%d, got %d", name,
           2 * NRS + 1, s);
    size_t lds = (size_t)(NPSZ + NNSZ + 2 * NHSZ) * sizeof(int) + (size_t)table_len * 2;
    int hbufs = 2;
    if (lds > (size_t)NLDS_MAX) {
        hbufs = 1;
        lds -= NHSZ * sizeof(int);
    }
    DG_ARG(table_len >= 1 && lds <= (size_t)NLDS_MAX, "%s: bad weight table length %d", name, table_len);
    if (n == 0) return DG_OK;
    DG_ARG(in && out && table, "%s: NULL tensor", name);
    DG_ARG(in != out, "%s: the output must not be the input", name);
    const dim3 grid(dg_cdiv(w, NTW), dg_cdiv(h, NTH), n);
    auto kernel = t == 3 ? k_nlm<3> : t == 5 ? k_nlm<5> : k_nlm<7>;
    hipLaunchKernelGGL(kernel, grid, dim3(NT), lds, (hipStream_t)stream, h, w, s / 2, hbufs, table, table_len, in, out);
    DG_LAUNCHED(name);
    return DG_OK;
}
