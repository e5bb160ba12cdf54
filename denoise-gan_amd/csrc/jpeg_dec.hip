// Baseline JPEG decoder (include/dgan.h "Baseline JPEG decoder"; the definition in numpy:
// dgan/jpeg.py jpeg_decode_ref).  The entropy decoder is a self-synchronising parallel Huffman
// decoder (Klein & Wiseman; Weissenberger & Schmidt 2018) on JPEG's state (bit position, block of
// the MCU, zigzag index): jpeg_huff.h decodes one subsequence of JD_SUB bytes from a given state,
// and a lane's state is right as soon as it is the state the lane before it ends in.
//   k_jd_unstuff  a workgroup per image: the scan without the 0x00 behind every 0xFF, compacted
//                 16 bytes per lane and trip through a workgroup scan; clears the status words
//   k_jd_ripple   a workgroup per JD_T subsequences.  It stages its JD_T * JD_SUB bytes and a row
//                 of spill into LDS by coalesced 16-byte loads, byte-swapped (a word's first bit
//                 highest) and bank-rotated per row, and the image's four code tables beside them.
//                 Round 0: every lane decodes from its subsequence's first bit in state (0, 0).
//                 Then lane i + 1 decodes again from lane i's end state until a trip over the
//                 workgroup changes no end state; lane 0 starts from the end state of the
//                 workgroup before (round r reads what round r - 1 wrote: two buffers), in
//                 round 0 from a guess.  A lane decodes again only when its start state changed.
//                 The host launches rounds until one changes nothing: by induction from
//                 subsequence 0, whose start is known, that fixed point is the sequential parse.
//                 Nothing waits on a flag; rounds are bounded by the workgroups of an image.
//   k_jd_scan     a workgroup per image: the exclusive scan of the blocks every subsequence
//                 completes; fewer than the image holds: status bit 0
//   k_jd_zero     clears the levels
//   k_jd_write    the ripple's staging again; every lane decodes from its final start state and
//                 stores the levels as int16 [image][block][64] in natural order, a symbol in the
//                 subsequence its first bit lies in (so two lanes may share a block)
//   k_jd_dc       a workgroup per (component, image): the inclusive scan of the DC differences
//   k_jd_idct     a workgroup per four MCUs, a lane per block column then row: dequantise with the
//                 component's table, both jidctint passes, the range limit, into the uint8 planes
//   k_jpeg_pixels jpeg.hip's, unchanged: upsampling and colour
// The blob, one upload from the host (dgan/jpeg.py _decode_blob), everything at multiples of 16
// bytes: per image a descriptor of JD_DESC_WORDS words {scan offset, scan bytes, offset of its four
// code tables, table selectors (bit 2c: component c's DC table, bit 2c + 1: its AC table), 192
// bytes of quantisation tables of Y, Cb, Cr in natural order}, the table sets, the scans, each
// followed by zero bytes up to a multiple of 16.  The kernels check every offset of a descriptor
// against the blob's size; whatever the scan's bytes are, block indices are checked against the
// image's blocks before a store and table indices are masked.
#include <algorithm>
#include "jpeg_back.h"
#include "jpeg_huff.h"

namespace dg {

constexpr int JD_DESC_WORDS = 4 + 48;
constexpr int JD_WT = 1024;   // threads of the per-image kernels (unstuff, scans)

__constant__ unsigned char c_jd_natural[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47,
    55, 62, 63};

struct JdArgs {
    int n, mx, my;
    long nblk;           // blocks of one image: mx * my * 6
    unsigned max_scan;   // bytes of the longest scan of the call
    unsigned S, G;       // subsequences / workgroups an image has at most
    long ustride;        // bytes between two unstuffed scans
    size_t blob_bytes;
    int *changed, *status;
    unsigned *ulen;      // [n] bytes of the unstuffed scans
    jd_state *bound;     // [2][n][G] the end state of every workgroup, by round parity
    jd_state *sin, *sexit;   // [n][S] start and end state of every subsequence
    unsigned *cnt, *boff;    // [n][S] blocks completed, and their exclusive scan
    unsigned char *U;
    short *coef;
    unsigned char *planes;
};

struct JdImage {
    bool ok;
    const unsigned char *scan;
    unsigned scan_len, sel;
    const unsigned *tabs, *quant;
};

__device__ __forceinline__ JdImage jd_image(const JdArgs &A, const unsigned char *blob, int img) {
    const unsigned *d = reinterpret_cast<const unsigned *>(blob) + (long)img * JD_DESC_WORDS;
    const unsigned off = d[0], len = d[1], toff = d[2];
    JdImage I;
    I.ok = len <= A.max_scan && (off & 15) == 0 && (toff & 15) == 0 &&
           (size_t)off + ((len + 15) & ~15u) <= A.blob_bytes && (size_t)toff + 16 * JD_TAB_WORDS <= A.blob_bytes;
    I.scan = blob + (I.ok ? off : 0);
    I.scan_len = I.ok ? len : 0;
    I.tabs = reinterpret_cast<const unsigned *>(blob + (I.ok ? toff : 0));
    I.sel = d[3];
    I.quant = d + 4;
    return I;
}

// the exclusive scan of v over the JD_WT threads of a workgroup; all: their sum
__device__ __forceinline__ unsigned jd_block_scan(unsigned v, unsigned *wsum, unsigned &all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    all = 0;
    for (int k = 0; k < JD_WT / 64; ++k) {
        if (k < wave) before += wsum[k];
        all += wsum[k];
    }
    __syncthreads();
    return before + inc - v;
}

// grid n
__global__ void __launch_bounds__(JD_WT)
k_jd_unstuff(JdArgs A, const unsigned char *__restrict__ blob) {
    __shared__ unsigned wsum[JD_WT / 64];
    const int img = blockIdx.x, t = threadIdx.x;
    const JdImage I = jd_image(A, blob, img);
    unsigned char *U = A.U + (long)img * A.ustride;
    unsigned carry = 0;
    for (unsigned base = 0; base < I.scan_len; base += JD_WT * 16) {   // (the same trips for every thread)
        const unsigned b0 = base + t * 16;
        uint4 q = make_uint4(0, 0, 0, 0);
        unsigned prev = 0;
        int nv = 0;
        if (b0 < I.scan_len) {   // the scan is padded to a multiple of 16 bytes
            q = *reinterpret_cast<const uint4 *>(I.scan + b0);
            prev = b0 ? I.scan[b0 - 1] : 0;
            nv = (int)min(16u, I.scan_len - b0);
        }
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        unsigned keep = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned b = (w[k >> 2] >> (8 * (k & 3))) & 255;
            if (k < nv && !(b == 0 && prev == 255)) keep |= 1u << k;
            prev = b;
        }
        unsigned all;
        unsigned o = carry + jd_block_scan(__popc(keep), wsum, all);   // o + popc(keep) <= scan_len <= ustride
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((keep >> k) & 1) U[o++] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
        carry += all;
    }
    if (t == 0) {
        A.ulen[img] = carry;
        A.status[img] = I.ok ? 0 : 4;
        if (img == 0) *A.changed = 0;
    }
}

// The workgroup's bytes [g * JD_T * JD_SUB, + JD_WORDS * 4) of the unstuffed scan into `words`, 0
// behind the scan's end, and the image's tables; ends with a barrier.
__device__ __forceinline__ void jd_stage(unsigned *words, unsigned *tabs, unsigned char *natural,
                                         const unsigned char *__restrict__ U, unsigned ulen, unsigned g,
                                         const JdImage &I) {
    const int t = threadIdx.x;
    const unsigned byte0 = g * (JD_T * JD_SUB);
    for (int i = t; i < JD_WORDS / 4; i += JD_T) {
        const unsigned o = byte0 + i * 16;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (o < ulen) q = *reinterpret_cast<const uint4 *>(U + o);   // ustride is a multiple of 16 above the scan
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long valid = (long)ulen - (long)(o + 4 * k);   // bytes of this word inside the scan
            unsigned v = __builtin_bswap32(w[k]);
            if (valid <= 0) v = 0;
            else if (valid < 4) v &= 0xffffffffu << (8 * (4 - (int)valid));
            words[jd_swizzle(i * 4 + k)] = v;
        }
    }
    for (int i = t; i < 4 * JD_TAB_WORDS; i += JD_T) tabs[i] = I.ok ? I.tabs[i] : 0;
    if (natural && t < 64) natural[t] = c_jd_natural[t];
    __syncthreads();
}

// a start state with its bit position inside [start, start + JD_SYMBOL_BITS]: where the lane
// before can end by construction
__device__ __forceinline__ jd_state jd_clamp(jd_state s, unsigned start) {
    const unsigned p = min(max((unsigned)s, start), start + JD_SYMBOL_BITS);
    return (s & ~0xffffffffull) | p;
}

// grid (G, n)
__global__ void __launch_bounds__(JD_T)
k_jd_ripple(JdArgs A, const unsigned char *__restrict__ blob, int round) {
    __shared__ unsigned words[JD_WORDS];
    __shared__ unsigned tabs[4 * JD_TAB_WORDS];
    __shared__ jd_state st[JD_T];
    const int img = blockIdx.y, t = threadIdx.x;
    const unsigned g = blockIdx.x;
    const unsigned ulen = min(A.ulen[img], A.max_scan), total = ulen * 8;
    const unsigned nsub = (ulen + JD_SUB - 1) / JD_SUB;
    if (g * JD_T >= nsub) return;   // (the whole workgroup)
    const JdImage I = jd_image(A, blob, img);
    jd_stage(words, tabs, nullptr, A.U + (long)img * A.ustride, ulen, g, I);

    const unsigned sub = g * JD_T + t, base = g * (JD_T * JD_SUB_BITS), start = sub * JD_SUB_BITS;
    const bool live = sub < nsub;
    const unsigned limit = min(start + JD_SUB_BITS, total);
    const long si = (long)img * A.S + sub;
    JdSink none{};
    jd_state in = jd_pack(start, 0, 0), ex = 0, old_ex = 0;
    int c = 0, old_c = 0;
    if (live) {
        if (round == 0) {
            ex = jd_decode(words, base, tabs, I.sel, in, limit, total, c, none);
        } else {
            in = A.sin[si];
            ex = old_ex = A.sexit[si];
            c = old_c = (int)A.cnt[si];
        }
    }
    const long nb = (long)A.n * A.G, bi = (long)img * A.G + g;
    const jd_state wg_in = g == 0 ? jd_pack(0, 0, 0) : round == 0 ? jd_pack(base, 0, 0) : A.bound[((round - 1) & 1) * nb + bi - 1];
    st[t] = ex;
    for (int trip = 0; trip < JD_T; ++trip) {   // lane k is final after trip k
        __syncthreads();
        const jd_state from = t == 0 ? wg_in : st[t - 1];
        __syncthreads();
        bool moved = false;
        if (live && from != in) {
            in = from;
            const jd_state e2 = jd_decode(words, base, tabs, I.sel, jd_clamp(in, start), limit, total, c, none);
            moved = e2 != ex;
            ex = e2;
            st[t] = ex;
        }
        if (!__syncthreads_or(moved)) break;
    }
    if (live) {
        A.sin[si] = in;
        A.sexit[si] = ex;
        A.cnt[si] = (unsigned)c;
        if (t == JD_T - 1 || sub == nsub - 1) A.bound[(round & 1) * nb + bi] = ex;
    }
    const bool changed = live && round > 0 && (ex != old_ex || c != old_c);
    if (__syncthreads_or(changed) && t == 0) atomicAdd(A.changed, 1);
}

// grid n
__global__ void __launch_bounds__(JD_WT)
k_jd_scan(JdArgs A) {
    __shared__ unsigned wsum[JD_WT / 64];
    const int img = blockIdx.x, t = threadIdx.x;
    const unsigned ulen = min(A.ulen[img], A.max_scan);
    const unsigned nsub = (ulen + JD_SUB - 1) / JD_SUB;
    const unsigned *src = A.cnt + (long)img * A.S;
    unsigned *dst = A.boff + (long)img * A.S;
    unsigned long long carry = 0;
    for (unsigned base = 0; base < nsub; base += JD_WT) {
        const unsigned v = base + t < nsub ? src[base + t] : 0;   // at most JD_SUB_BITS / 2 each
        unsigned all;
        const unsigned before = jd_block_scan(v, wsum, all);
        if (base + t < nsub) dst[base + t] = (unsigned)min(carry + before, 0xffffffffull);
        carry += all;
    }
    if (t == 0 && carry < (unsigned long long)A.nblk) atomicOr(A.status + img, 1);
}

__global__ void __launch_bounds__(JD_T)
k_jd_zero(uint4 *__restrict__ p, long count) {
    for (long i = (long)blockIdx.x * JD_T + threadIdx.x; i < count; i += (long)gridDim.x * JD_T)
        p[i] = make_uint4(0, 0, 0, 0);
}

// grid (G, n)
__global__ void __launch_bounds__(JD_T)
k_jd_write(JdArgs A, const unsigned char *__restrict__ blob) {
    __shared__ unsigned words[JD_WORDS];
    __shared__ unsigned tabs[4 * JD_TAB_WORDS];
    __shared__ unsigned char natural[64];
    const int img = blockIdx.y, t = threadIdx.x;
    const unsigned g = blockIdx.x;
    const unsigned ulen = min(A.ulen[img], A.max_scan), total = ulen * 8;
    const unsigned nsub = (ulen + JD_SUB - 1) / JD_SUB;
    if (g * JD_T >= nsub) return;   // (the whole workgroup)
    const JdImage I = jd_image(A, blob, img);
    jd_stage(words, tabs, natural, A.U + (long)img * A.ustride, ulen, g, I);
    const unsigned sub = g * JD_T + t, base = g * (JD_T * JD_SUB_BITS), start = sub * JD_SUB_BITS;
    if (sub >= nsub) return;
    const long si = (long)img * A.S + sub;
    JdSink sink{A.coef + (long)img * A.nblk * 64, (long)A.boff[si], A.nblk, natural, false};
    int c;
    jd_decode(words, base, tabs, I.sel, jd_clamp(A.sin[si], start), min(start + JD_SUB_BITS, total), total, c, sink);
    if (sink.short_of_bits) atomicOr(A.status + img, 2);
}

// grid (3, n): DC differences -> DC levels, per component in scan order (Y: four blocks per MCU)
__global__ void __launch_bounds__(JD_WT)
k_jd_dc(JdArgs A) {
    __shared__ unsigned wsum[JD_WT / 64];
    const int comp = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    short *coef = A.coef + (long)img * A.nblk * 64;
    const long mcus = A.nblk / 6, count = comp == 0 ? 4 * mcus : mcus;
    unsigned carry = 0;   // sums wrap like the int16 they are stored as
    for (long base = 0; base < count; base += JD_WT) {
        const long j = base + t;
        const long blk = comp == 0 ? (j >> 2) * 6 + (j & 3) : j * 6 + 3 + comp;
        const unsigned v = j < count ? (unsigned)(int)coef[blk * 64] : 0;
        unsigned all;
        const unsigned before = jd_block_scan(v, wsum, all);
        if (j < count) coef[blk * 64] = (short)(carry + before + v);
        carry += all;
    }
}

// grid (ceil(MCUs / 4), n): lane t holds column t & 7, then row t & 7, of block t >> 3 of 24
__global__ void __launch_bounds__(JT)
k_jd_idct(JdArgs A, JpegArgs P, const unsigned char *__restrict__ blob) {
    __shared__ int buf[JT * JLD];
    const int img = blockIdx.y, t = threadIdx.x;
    const int b = t >> 3, c = t & 7;
    const long mcus = A.nblk / 6, m = (long)blockIdx.x * 4 + b / 6;
    const int idx = b % 6, comp = idx < 4 ? 0 : idx - 3;
    const bool live = m < mcus;
    const unsigned char *qt = reinterpret_cast<const unsigned char *>(
        reinterpret_cast<const unsigned *>(blob) + (long)img * JD_DESC_WORDS + 4) + comp * 64;
    int d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = 0;
    if (live) {
        const short *src = A.coef + ((long)img * A.nblk + m * 6 + idx) * 64;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)src[k * 8 + c] * (int)qt[k * 8 + c];
    }
    jpeg_idct8<true>(d);
    int *col = buf + b * 8 * JLD + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k * JLD] = d[k];
    __syncthreads();
    const int *row = buf + t * JLD;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = row[k];
    jpeg_idct8<false>(d);
    if (!live) return;
    uint2 v;
    v.x = jpeg_limit(d[0]) | (jpeg_limit(d[1]) << 8) | (jpeg_limit(d[2]) << 16) | (jpeg_limit(d[3]) << 24);
    v.y = jpeg_limit(d[4]) | (jpeg_limit(d[5]) << 8) | (jpeg_limit(d[6]) << 16) | (jpeg_limit(d[7]) << 24);
    // A.my * 16 == P.Hp and A.mx * 16 <= P.Wp: every block lies inside the planes, at a multiple of 8
    unsigned char *planes = A.planes + (long)img * jpeg_image_bytes(P.Hp, P.Wp);
    const int my = (int)(m / A.mx), mx = (int)(m % A.mx), r = t & 7;
    unsigned char *dst;
    if (idx < 4) {
        dst = planes + (long)(my * 16 + (idx >> 1) * 8 + r) * P.Wp + mx * 16 + (idx & 1) * 8;
    } else {
        const int Hc = P.Hp / 2, Wc = P.Wp / 2;
        dst = planes + (long)P.Hp * P.Wp + (long)(idx - 4) * Hc * Wc + (long)(my * 8 + r) * Wc + mx * 8;
    }
    *reinterpret_cast<uint2 *>(dst) = v;
}

static size_t jd_up16(size_t v) { return (v + 15) / 16 * 16; }

// the geometry of a call and its workspace: `ws` NULL sizes it
static int jd_setup(const char *name, int n, int h, int w, long long max_scan, void *ws, JpegArgs &P, JdArgs &A,
                    size_t &bytes) {
    if (int rc = jpeg_shape(name, n, h, w, P)) return rc;
    DG_ARG(h <= 65535 && w <= 65535, "%s: bad shape: a JPEG file holds 1..65535 rows and columns, got %dx%d", name, h, w);
    DG_ARG(max_scan >= 0 && max_scan < (1LL << 28), "%s: a scan of %lld bytes, at most 2^28 - 1", name, max_scan);
    A.n = n;
    A.mx = (w + 15) / 16;
    A.my = (h + 15) / 16;
    A.nblk = (long)A.mx * A.my * 6;
    DG_ARG(A.nblk * n <= (1L << 30), "%s: bad shape: %ld blocks in one call, at most 2^30", name, A.nblk * n);
    A.max_scan = (unsigned)max_scan;
    A.S = std::max(1u, (A.max_scan + JD_SUB - 1) / JD_SUB);
    A.G = (A.S + JD_T - 1) / JD_T;
    A.ustride = (long)jd_up16((size_t)max_scan) + 16;
    char *p = (char *)ws;
    size_t at = 0;
    auto take = [&](size_t b) { char *q = p + at; at += jd_up16(b); return q; };
    A.changed = (int *)take(4);
    A.status = (int *)take((size_t)n * 4);
    A.ulen = (unsigned *)take((size_t)n * 4);
    A.bound = (jd_state *)take((size_t)2 * n * A.G * 8);
    A.sin = (jd_state *)take((size_t)n * A.S * 8);
    A.sexit = (jd_state *)take((size_t)n * A.S * 8);
    A.cnt = (unsigned *)take((size_t)n * A.S * 4);
    A.boff = (unsigned *)take((size_t)n * A.S * 4);
    A.U = (unsigned char *)take((size_t)n * A.ustride);
    A.coef = (short *)take((size_t)n * A.nblk * 128);
    A.planes = (unsigned char *)take((size_t)n * (size_t)jpeg_image_bytes(P.Hp, P.Wp));
    bytes = at;
    return DG_OK;
}

static int jd_call(const char *name, int n, int h, int w, const void *blob, size_t blob_bytes, long long max_scan,
                   void *ws, size_t ws_bytes, JpegArgs &P, JdArgs &A) {
    size_t need;
    if (int rc = jd_setup(name, n, h, w, max_scan, ws, P, A, need)) return rc;
    if (n == 0) return DG_OK;
    DG_ARG(blob && ws, "%s: NULL tensor", name);
    DG_ARG(blob_bytes >= (size_t)n * JD_DESC_WORDS * 4, "%s: a blob of %zu bytes holds no %d descriptors", name,
           blob_bytes, n);
    DG_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", name, ws_bytes, need);
    DG_ARG((((uintptr_t)ws) & 15) == 0 && (((uintptr_t)blob) & 15) == 0, "%s: the blob and the workspace must be 16-byte aligned",
           name);
    A.blob_bytes = blob_bytes;
    return DG_OK;
}

}  // namespace dg

int dg_jpeg_decode_geometry(int *subsequence_bytes, int *lanes) {
    DG_ARG(subsequence_bytes && lanes, "jpeg_decode_geometry: NULL result");
    *subsequence_bytes = dg::JD_SUB;
    *lanes = dg::JD_T;
    return DG_OK;
}

int dg_jpeg_decode_ws_bytes(int n, int h, int w, long long max_scan_bytes, size_t *bytes) {
    dg::JpegArgs P;
    dg::JdArgs A;
    DG_ARG(bytes, "jpeg_decode_ws_bytes: NULL result");
    return dg::jd_setup("jpeg_decode_ws_bytes", n, h, w, max_scan_bytes, nullptr, P, A, *bytes);
}

int dg_jpeg_decode_scan(int n, int h, int w, const void *blob, size_t blob_bytes, long long max_scan_bytes, void *ws,
                        size_t ws_bytes, dg_stream_t stream) {
    using namespace dg;
    JpegArgs P;
    JdArgs A;
    if (int rc = jd_call("jpeg_decode_scan", n, h, w, blob, blob_bytes, max_scan_bytes, ws, ws_bytes, P, A)) return rc;
    if (n == 0) return DG_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_jd_unstuff, dim3(n), dim3(JD_WT), 0, s, A, (const unsigned char *)blob);
    DG_LAUNCHED("jpeg_decode_scan (unstuff)");
    hipLaunchKernelGGL(k_jd_ripple, dim3(A.G, n), dim3(JD_T), 0, s, A, (const unsigned char *)blob, 0);
    DG_LAUNCHED("jpeg_decode_scan (decode)");
    return DG_OK;
}

int dg_jpeg_decode_sync(int n, int h, int w, const void *blob, size_t blob_bytes, long long max_scan_bytes, void *ws,
                        size_t ws_bytes, int round, dg_stream_t stream) {
    using namespace dg;
    JpegArgs P;
    JdArgs A;
    if (int rc = jd_call("jpeg_decode_sync", n, h, w, blob, blob_bytes, max_scan_bytes, ws, ws_bytes, P, A)) return rc;
    DG_ARG(round >= 1, "jpeg_decode_sync: round %d, the first is 1", round);
    if (n == 0) return DG_OK;
    hipLaunchKernelGGL(k_jd_ripple, dim3(A.G, n), dim3(JD_T), 0, (hipStream_t)stream, A, (const unsigned char *)blob,
                       round);
    DG_LAUNCHED("jpeg_decode_sync");
    return DG_OK;
}

int dg_jpeg_decode_pixels(int n, int h, int w, const void *blob, size_t blob_bytes, long long max_scan_bytes, void *ws,
                          size_t ws_bytes, unsigned char *out, dg_stream_t stream) {
    using namespace dg;
    JpegArgs P;
    JdArgs A;
    if (int rc = jd_call("jpeg_decode_pixels", n, h, w, blob, blob_bytes, max_scan_bytes, ws, ws_bytes, P, A)) return rc;
    if (n == 0) return DG_OK;
    DG_ARG(out, "jpeg_decode_pixels: NULL tensor");
    hipStream_t s = (hipStream_t)stream;
    const unsigned char *b = (const unsigned char *)blob;
    hipLaunchKernelGGL(k_jd_scan, dim3(n), dim3(JD_WT), 0, s, A);
    DG_LAUNCHED("jpeg_decode_pixels (scan)");
    const long quads = (long)n * A.nblk * 8;
    hipLaunchKernelGGL(k_jd_zero, dim3((unsigned)std::min<long>(dg_cdiv(quads, JD_T), 4096)), dim3(JD_T), 0, s,
                       (uint4 *)A.coef, quads);
    DG_LAUNCHED("jpeg_decode_pixels (zero)");
    hipLaunchKernelGGL(k_jd_write, dim3(A.G, n), dim3(JD_T), 0, s, A, b);
    DG_LAUNCHED("jpeg_decode_pixels (levels)");
    hipLaunchKernelGGL(k_jd_dc, dim3(3, n), dim3(JD_WT), 0, s, A);
    DG_LAUNCHED("jpeg_decode_pixels (dc)");
    hipLaunchKernelGGL(k_jd_idct, dim3(dg_cdiv(A.nblk / 6, 4), n), dim3(JT), 0, s, A, P, b);
    DG_LAUNCHED("jpeg_decode_pixels (idct)");
    return jpeg_launch_pixels("jpeg_decode_pixels (pixels)", P, n, A.planes, out, s);
}
