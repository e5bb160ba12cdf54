// PNG encoder for 8-bit RGB frames (include/dgan.h "PNG encoder"; the definition in numpy:
// dgan/png.py png_encode_ref, whose module docstring fixes the format).  Four launches, integers only:
//   k_png_filter  a workgroup per row: the five filters' sums of min(v, 256 - v) in one pass over the
//                 row and the row above, then the winner's bytes into the filtered stream
//   k_png_block   a workgroup of 1024 threads per span of 32768 stream bytes, 32 consecutive bytes per
//                 thread, the span in LDS.  Run starts as a 32-bit mask per thread; the start of the
//                 run a thread enters in and the start of the next run after it by a max scan and a
//                 reversed min scan over the threads; every byte's token from the rule's closed form
//                 (position in its run, run length); LDS histogram; the used symbols ranked by
//                 (count, symbol) in parallel, then one lane runs the two-queue merge, the depth
//                 count, the Kraft repair and the canonical codes, and codes the header's lengths;
//                 every thread's token bits, their exclusive scan, the stored-or-dynamic decision;
//                 the codes ORed first bit lowest into the LDS output buffer through a 64-bit
//                 accumulator per thread; the span's Adler-32 parts (sum, position-weighted sum) and
//                 the chunk's CRC-32: every thread the register of its slice from 0, multiplied by
//                 x^(8 bytes after the slice) mod P, all XORed
//   k_png_scan    a workgroup per image: the chunks' offsets in the file, the Adler-32 of the whole
//                 stream from the spans' parts (a' = a + A, b' = b + n a + B: two prefix sums), the
//                 last chunk's CRC, the file's length
//   k_png_pack    a workgroup per chunk: length, type, payload and CRC at the chunk's offset, dwords
//                 where the destination is aligned; one more per image for signature, IHDR (host
//                 bytes by value), the last IDAT chunk and IEND
// dg_png_deflate runs the last three on any bytes and leaves the chunk framing out: a zlib stream.
// LDS of k_png_block: span 32768 + output 32800 + scan 4096 + counts, codes, lengths, the merge's
// queues and the header's items 12.5 K = about 80 KiB of the CU's 160.
#include <algorithm>
#include "common.h"

namespace dg {

constexpr int PN_SPAN = 32768;
constexpr int PN_T = 1024;                 // threads of k_png_block
constexpr int PN_PER = PN_SPAN / PN_T;     // stream bytes of a thread: the bits of its run-start mask
constexpr int PN_ROOM = 32784;             // bytes a block has in the workspace: stored, 5 + 32768, to 16
constexpr int PN_OBUF = PN_ROOM / 4 + 4;   // dwords of the LDS output buffer: the accumulator's last flush
constexpr int PN_META = 4;                 // words per span: payload bytes, Adler A, Adler B, CRC
constexpr int PN_SYM = 288;                // room of the literal/length alphabet (286)
constexpr int PN_PT = 256;                 // threads of the filter, scan and pack kernels
constexpr int PN_HDR = 40;                 // most bytes before the first IDAT chunk (33 are written)
constexpr unsigned PN_POLY = 0xedb88320u;
constexpr unsigned PN_ADLER = 65521;
static_assert(PN_PER == 32, "a thread's run starts are one 32-bit mask");

__constant__ unsigned char c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PngHeader {
    unsigned char b[PN_HDR];
};

// ---- CRC-32 as polynomials mod P, bit 31 the coefficient of x^0 -------------------------------------
__device__ __forceinline__ unsigned crc_byte(unsigned c, unsigned byte) {
    c ^= byte;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c >> 1) ^ ((c & 1) ? PN_POLY : 0);
    return c;
}

__device__ __forceinline__ unsigned crc_mul(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? PN_POLY : 0);
    }
    return p;
}

__device__ __forceinline__ unsigned crc_xpow8(unsigned k) {   // x^(8 k)
    unsigned r = 0x80000000u, b = 0x00800000u;
    for (; k; k >>= 1) {
        if (k & 1) r = crc_mul(r, b);
        b = crc_mul(b, b);
    }
    return r;
}

// ---- the filter ------------------------------------------------------------------------------------
__device__ __forceinline__ int png_filtered(int type, int x, int a, int b, int c) {
    int pred = 0;
    if (type == 1) pred = a;
    else if (type == 2) pred = b;
    else if (type == 3) pred = (a + b) >> 1;
    else if (type == 4) {
        const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x - pred) & 255;
}

// grid (h, n).  filt: n streams `stride` bytes apart
__global__ void __launch_bounds__(PN_PT)
k_png_filter(int h, int w, const unsigned char *__restrict__ in, unsigned char *__restrict__ filt, long stride) {
    __shared__ unsigned wsum[PN_PT / 64][5];
    const int y = blockIdx.x, t = threadIdx.x, rb = 3 * w;
    const unsigned char *cur = in + ((long)blockIdx.y * h + y) * rb;
    const unsigned char *prev = cur - rb;   // read for y > 0 only
    unsigned s[5] = {0, 0, 0, 0, 0};
    for (int i = t; i < rb; i += PN_PT) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y ? prev[i] : 0, c = (y && i >= 3) ? prev[i - 3] : 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            const int v = png_filtered(f, x, a, b, c);
            s[f] += min(v, 256 - v);
        }
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s[f] += __shfl_xor(s[f], o);
        if ((t & 63) == 0) wsum[t >> 6][f] = s[f];
    }
    __syncthreads();
    int best = 0;
    unsigned least = 0;
    for (int f = 0; f < 5; ++f) {
        unsigned v = 0;
        for (int k = 0; k < PN_PT / 64; ++k) v += wsum[k][f];
        if (f == 0 || v < least) {   // a tie: the lower type stays
            least = v;
            best = f;
        }
    }
    unsigned char *dst = filt + (long)blockIdx.y * stride + (long)y * (rb + 1);
    if (t == 0) dst[0] = (unsigned char)best;
    for (int i = t; i < rb; i += PN_PT) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y ? prev[i] : 0, c = (y && i >= 3) ? prev[i - 3] : 0;
        dst[1 + i] = (unsigned char)png_filtered(best, x, a, b, c);
    }
}

// ---- the block kernel's parts ----------------------------------------------------------------------
struct PngMax {
    __device__ unsigned operator()(unsigned a, unsigned b) const { return max(a, b); }
};
struct PngMin {
    __device__ unsigned operator()(unsigned a, unsigned b) const { return min(a, b); }
};
struct PngAdd {
    __device__ unsigned operator()(unsigned a, unsigned b) const { return a + b; }
};

// The scan of v over the workgroup's threads, from thread 0 up or (rev) from the last one down: returns
// the value of the threads before this one (ident for the first), `all` the value of all.  Every thread
// calls it; tmp: PN_T words.
template <class Op>
__device__ __forceinline__ unsigned png_scan(unsigned v, unsigned *tmp, Op op, bool rev, unsigned ident, unsigned &all) {
    const int j = rev ? PN_T - 1 - (int)threadIdx.x : (int)threadIdx.x;
    __syncthreads();
    tmp[j] = v;
    for (int o = 1; o < PN_T; o <<= 1) {
        __syncthreads();
        const unsigned u = j >= o ? tmp[j - o] : ident;
        __syncthreads();
        if (j >= o) {
            v = op(v, u);
            tmp[j] = v;
        }
    }
    __syncthreads();
    all = tmp[PN_T - 1];
    return j ? tmp[j - 1] : ident;
}

struct PngToken {
    int sym;      // literal/length symbol, -1: the byte lies inside a match
    int eb, ev;   // extra bits and their value
};

// The token of byte `pos` of value v, whose run starts at rs and ends before ne (dgan/png.py _tokens)
__device__ __forceinline__ PngToken png_token(int pos, int v, int rs, int ne) {
    PngToken k = {v, 0, 0};
    const int q = pos - rs - 1, R = ne - rs - 1;
    if (q < 0) return k;
    const int full = R / 258 * 258;
    int len;
    if (q < full) len = q % 258 == 0 ? 258 : 0;
    else if (R - full >= 3) len = q == full ? R - full : 0;
    else return k;
    if (len == 0) {
        k.sym = -1;
        return k;
    }
    const int l3 = len - 3;
    if (len == 258) k.sym = 285;
    else if (l3 < 8) k.sym = 257 + l3;
    else {
        k.eb = 29 - __clz(l3);   // floor(log2 l3) - 2
        k.sym = 261 + 4 * k.eb + ((l3 >> k.eb) & 3);
        k.ev = l3 & ((1 << k.eb) - 1);
    }
    return k;
}

// A thread's view of its 32 bytes: where the runs around them start
struct PngRuns {
    int base, nv;        // first byte, bytes inside the span
    unsigned fm;         // bit k: byte base + k starts a run
    int rs_in, ne_in;    // the start of the run byte `base` continues; the first start after the thread's bytes
    __device__ __forceinline__ void around(int k, int &rs, int &ne) const {
        const unsigned lower = fm & (0xffffffffu >> (31 - k));
        const unsigned upper = k == 31 ? 0u : fm & (0xffffffffu << (k + 1));
        rs = lower ? base + 31 - __clz(lower) : rs_in;
        ne = upper ? base + __ffs(upper) - 1 : ne_in;
    }
};

struct PngScratch {   // the code builder's: sorted weights and symbols, the merged nodes, parents, depths
    unsigned sw[PN_SYM], nw[PN_SYM];
    unsigned short ss[PN_SYM], lp[PN_SYM], np[PN_SYM], dp[PN_SYM];
    unsigned used;
};

// cnt[nsym] -> lens[nsym], at most `limit` bits (dgan/png.py code_lengths).  Every thread calls it.
__device__ void png_code_lengths(const unsigned *cnt, int nsym, int limit, unsigned char *lens, PngScratch &S) {
    const int t = threadIdx.x;
    if (t == 0) S.used = 0;
    __syncthreads();
    if (t < nsym) {
        lens[t] = 0;
        const unsigned c = cnt[t];
        if (c) {
            int rank = 0;
            for (int j = 0; j < nsym; ++j) {
                const unsigned cj = cnt[j];
                rank += cj && (cj < c || (cj == c && j < t));
            }
            S.sw[rank] = c;
            S.ss[rank] = (unsigned short)t;
            atomicAdd(&S.used, 1u);
        }
    }
    __syncthreads();
    if (t == 0) {
        const int n = (int)S.used;
        if (n == 1) lens[S.ss[0]] = 1;
        if (n >= 2) {
            int li = 0, ni = 0;
            for (int k = 0; k < n - 1; ++k) {   // the leaf when the heads weigh the same
                unsigned weight = 0;
                for (int rep = 0; rep < 2; ++rep) {
                    if (li < n && (ni >= k || S.sw[li] <= S.nw[ni])) {
                        weight += S.sw[li];
                        S.lp[li++] = (unsigned short)k;
                    } else {
                        weight += S.nw[ni];
                        S.np[ni++] = (unsigned short)k;
                    }
                }
                S.nw[k] = weight;
            }
            S.dp[n - 2] = 0;
            for (int k = n - 3; k >= 0; --k) S.dp[k] = S.dp[S.np[k]] + 1;
            int per[16];
            for (int b = 0; b < 16; ++b) per[b] = 0;
            for (int i = 0; i < n; ++i) per[min((int)S.dp[S.lp[i]] + 1, limit)]++;
            int kraft = 0;
            for (int b = 1; b <= limit; ++b) kraft += per[b] << (limit - b);
            while (kraft > (1 << limit)) {
                per[limit]--;
                int b = limit - 1;
                while (!per[b]) --b;
                per[b]--;
                per[b + 1] += 2;
                --kraft;
            }
            int i = 0;
            for (int b = limit; b >= 1; --b)
                for (int c = 0; c < per[b]; ++c) lens[S.ss[i++]] = (unsigned char)b;
        }
    }
    __syncthreads();
}

// One lane: the canonical codes of lens[nsym], every code's first bit lowest
__device__ void png_codes(const unsigned char *lens, int nsym, unsigned short *codes) {
    int per[17], nxt[17];
    for (int b = 0; b < 17; ++b) per[b] = 0;
    for (int s = 0; s < nsym; ++s) per[lens[s]]++;
    per[0] = 0;
    int code = 0;
    nxt[0] = 0;
    for (int b = 1; b < 17; ++b) {
        code = (code + per[b - 1]) << 1;
        nxt[b] = code;
    }
    for (int s = 0; s < nsym; ++s) {
        const int b = lens[s];
        codes[s] = b ? (unsigned short)(__brev((unsigned)nxt[b]++) >> (32 - b)) : 0;
    }
}

__device__ __forceinline__ void png_put(unsigned *obuf, unsigned pos, unsigned val, int nb) {   // nb <= 32
    const unsigned long long v = (unsigned long long)val << (pos & 31);
    atomicOr(obuf + (pos >> 5), (unsigned)v);
    if ((pos & 31) + nb > 32) atomicOr(obuf + (pos >> 5) + 1, (unsigned)(v >> 32));
}

// grid (spans, n).  data: n streams of `len` bytes, `stride` apart; span s of image i leaves its block
// at blocks + (i spans + s) PN_ROOM and its PN_META words at meta; framed: a PNG chunk's CRC is wanted
__global__ void __launch_bounds__(PN_T)
k_png_block(const unsigned char *__restrict__ data, long len, long stride, int framed, unsigned char *__restrict__ blocks,
            unsigned *__restrict__ meta) {
    __shared__ uint4 span4[PN_SPAN / 16];
    __shared__ __attribute__((aligned(16))) unsigned obuf[PN_OBUF];
    __shared__ unsigned tmp[PN_T];
    __shared__ unsigned hist[PN_SYM], clhist[19], items[PN_SYM];
    __shared__ unsigned short codes[PN_SYM], clcodes[19];
    __shared__ unsigned char lens[PN_SYM], cllens[19];
    __shared__ PngScratch S;
    __shared__ unsigned sh_adler[2], sh_crc, sh_hdr_bits, sh_items, sh_nlit, sh_ncl;
    unsigned char *span = reinterpret_cast<unsigned char *>(span4);
    const unsigned *span32 = reinterpret_cast<const unsigned *>(span4);
    const int t = threadIdx.x;
    const long at = (long)blockIdx.x * PN_SPAN;
    const int n = (int)min((long)PN_SPAN, len - at);   // >= 1: the host launches ceil(len / PN_SPAN) spans
    const unsigned char *src = data + (long)blockIdx.y * stride + at;

    int whole = 0;   // bytes loaded as 16-byte groups
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        whole = n & ~15;
        for (int i = t; i < whole / 16; i += PN_T) span4[i] = reinterpret_cast<const uint4 *>(src)[i];
    }
    for (int i = whole + t; i < n; i += PN_T) span[i] = src[i];
    for (int i = t; i < PN_SYM; i += PN_T) hist[i] = 0;
    for (int i = t; i < PN_OBUF; i += PN_T) obuf[i] = 0;
    if (t < 19) clhist[t] = 0;
    if (t < 2) sh_adler[t] = 0;
    if (t == 0) sh_crc = 0;
    __syncthreads();

    // run starts
    PngRuns r;
    r.base = t * PN_PER;
    r.nv = max(0, min(PN_PER, n - r.base));
    r.fm = 0;
    {
        int before = r.base > 0 && r.nv > 0 ? span[r.base - 1] : -1;
        for (int k = 0; k < r.nv; ++k) {
            const int v = span[r.base + k];
            r.fm |= (unsigned)(v != before) << k;
            before = v;
        }
    }
    unsigned all;
    r.rs_in = (int)png_scan(r.fm ? (unsigned)(r.base + 31 - __clz(r.fm)) : 0u, tmp, PngMax(), false, 0u, all);
    r.ne_in = (int)min((unsigned)n, png_scan(r.fm ? (unsigned)(r.base + __ffs(r.fm) - 1) : 0xffffffffu, tmp, PngMin(),
                                             true, 0xffffffffu, all));

    // counts and the Adler parts
    {
        unsigned sa = 0, sb = 0;
        for (int j = 0; j < PN_PER / 4; ++j) {
            const unsigned wd = span32[r.base / 4 + j];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = 4 * j + b;
                if (k < r.nv) {
                    const int v = (wd >> (8 * b)) & 255;
                    int rs, ne;
                    r.around(k, rs, ne);
                    const PngToken tk = png_token(r.base + k, v, rs, ne);
                    if (tk.sym >= 0) atomicAdd(&hist[tk.sym], 1u);
                    sa += v;
                    sb += (unsigned)(n - r.base - k) * v;
                }
            }
        }
        if (r.nv) {
            atomicAdd(&sh_adler[0], sa);                 // at most 1024 * 32 * 255
            atomicAdd(&sh_adler[1], sb % PN_ADLER);      // sb itself at most 32 * 32768 * 255
        }
        if (t == 0) hist[256] = 1;
    }
    __syncthreads();
    png_code_lengths(hist, 286, 15, lens, S);

    // one lane: the codes, the header's items, the code-length code's counts
    if (t == 0) {
        png_codes(lens, 286, codes);
        int nlit = 286, matches = 0;
        while (!lens[nlit - 1]) --nlit;   // stops at 256 or above
        for (int s = 257; s < 286; ++s) matches |= lens[s];
        lens[nlit] = matches ? 1 : 0;     // the distance code, the sequence's last entry (PN_SYM > 286)
        int ni = 0;
        for (int i = 0; i <= nlit;) {
            int j = i;
            const unsigned v = lens[i];
            while (j <= nlit && lens[j] == v) ++j;
            int left = j - i;
            if (v == 0) {
                while (left >= 11) {
                    const int m = min(left, 138);
                    items[ni++] = 18u | (7u << 8) | ((unsigned)(m - 11) << 16);
                    left -= m;
                }
                if (left >= 3) {
                    items[ni++] = 17u | (3u << 8) | ((unsigned)(left - 3) << 16);
                    left = 0;
                }
            } else {
                items[ni++] = v;
                --left;
                while (left >= 3) {
                    const int m = min(left, 6);
                    items[ni++] = 16u | (2u << 8) | ((unsigned)(m - 3) << 16);
                    left -= m;
                }
            }
            for (; left > 0; --left) items[ni++] = v;
            i = j;
        }
        for (int i = 0; i < ni; ++i) clhist[items[i] & 255]++;
        sh_items = ni;
        sh_nlit = nlit;
    }
    __syncthreads();
    png_code_lengths(clhist, 19, 7, cllens, S);
    if (t == 0) {
        png_codes(cllens, 19, clcodes);
        int ncl = 19;
        while (ncl > 4 && !cllens[c_cl_order[ncl - 1]]) --ncl;
        unsigned bits = 17 + 3 * ncl;
        for (int i = 0; i < (int)sh_items; ++i) bits += cllens[items[i] & 255] + ((items[i] >> 8) & 255);
        sh_ncl = ncl;
        sh_hdr_bits = bits;
    }
    __syncthreads();

    // token bits, their scan, the decision
    unsigned mine = 0;
    for (int j = 0; j < PN_PER / 4; ++j) {
        const unsigned wd = span32[r.base / 4 + j];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = 4 * j + b;
            if (k < r.nv) {
                int rs, ne;
                r.around(k, rs, ne);
                const PngToken tk = png_token(r.base + k, (wd >> (8 * b)) & 255, rs, ne);
                if (tk.sym >= 0) mine += lens[tk.sym] + tk.eb + (tk.sym > 256);
            }
        }
    }
    const unsigned before = png_scan(mine, tmp, PngAdd(), false, 0u, all);
    const unsigned bits = sh_hdr_bits + all + lens[256];
    const int dyn_bytes = (int)((bits + 3 + 7) / 8) + 4, stored_bytes = 5 + n;
    const bool dynamic = dyn_bytes < stored_bytes;   // (the same in every thread)
    const int nbytes = dynamic ? dyn_bytes : stored_bytes;
    unsigned char *ob = reinterpret_cast<unsigned char *>(obuf);

    if (dynamic) {
        if (t == 0) {   // BFINAL 0, BTYPE 2, HLIT, HDIST 0, HCLEN, the code-length code, the lengths
            unsigned pos = 0;
            png_put(obuf, pos, 2u << 1, 3);
            png_put(obuf, pos + 3, sh_nlit - 257, 5);
            png_put(obuf, pos + 13, sh_ncl - 4, 4);
            pos = 17;
            for (int k = 0; k < (int)sh_ncl; ++k, pos += 3) png_put(obuf, pos, cllens[c_cl_order[k]], 3);
            for (int i = 0; i < (int)sh_items; ++i) {
                const unsigned it = items[i], s = it & 255, cb = cllens[s], eb = (it >> 8) & 255;
                png_put(obuf, pos, clcodes[s] | ((it >> 16) << cb), cb + eb);
                pos += cb + eb;
            }
        }
        // this thread's tokens: an accumulator whose bit 0 is bit 0 of dword `word`
        unsigned pos = sh_hdr_bits + before;
        unsigned word = pos >> 5;
        int fill = pos & 31;
        unsigned long long acc = 0;
        for (int j = 0; j < PN_PER / 4; ++j) {
            const unsigned wd = span32[r.base / 4 + j];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = 4 * j + b;
                if (k < r.nv) {
                    int rs, ne;
                    r.around(k, rs, ne);
                    const PngToken tk = png_token(r.base + k, (wd >> (8 * b)) & 255, rs, ne);
                    if (tk.sym >= 0) {   // at most 15 + 5 + 1 bits: the distance code is one 0 bit
                        const int cb = lens[tk.sym];
                        acc |= (unsigned long long)(codes[tk.sym] | ((unsigned)tk.ev << cb)) << fill;
                        fill += cb + tk.eb + (tk.sym > 256);
                        if (fill >= 32) {
                            atomicOr(obuf + word++, (unsigned)acc);
                            acc >>= 32;
                            fill -= 32;
                        }
                    }
                }
            }
        }
        if (t == PN_T - 1) {   // the end-of-block symbol follows the last token
            acc |= (unsigned long long)codes[256] << fill;
            fill += lens[256];
        }
        if (fill > 0) {
            atomicOr(obuf + word, (unsigned)acc);
            if (fill > 32) atomicOr(obuf + word + 1, (unsigned)(acc >> 32));
        }
        __syncthreads();
        if (t == 0) {   // the empty stored block: its three bits and the padding are zeros already
            ob[dyn_bytes - 2] = 0xff;
            ob[dyn_bytes - 1] = 0xff;
        }
    } else {
        if (t == 0) {
            ob[0] = 0;
            ob[1] = (unsigned char)(n & 255);
            ob[2] = (unsigned char)(n >> 8);
            ob[3] = (unsigned char)(~n & 255);
            ob[4] = (unsigned char)((~n >> 8) & 255);
        }
        for (int k = 0; k < r.nv; ++k) ob[5 + r.base + k] = span[r.base + k];
    }
    __syncthreads();

    const bool first = blockIdx.x == 0;   // the first chunk's payload starts with the zlib header
    if (framed) {
        const int slice = (nbytes + PN_T - 1) / PN_T, b0 = min(nbytes, t * slice), b1 = min(nbytes, b0 + slice);
        unsigned c = 0;
        for (int i = b0; i < b1; ++i) c = crc_byte(c, ob[i]);
        if (c) atomicXor(&sh_crc, crc_mul(c, crc_xpow8((unsigned)(nbytes - b1))));
        __syncthreads();
        if (t == 0) {
            unsigned reg = 0xffffffffu;
            const unsigned char lead[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
            for (int i = 0; i < (first ? 6 : 4); ++i) reg = crc_byte(reg, lead[i]);
            sh_crc ^= crc_mul(reg, crc_xpow8((unsigned)nbytes));
        }
        __syncthreads();
    }
    const long g = (long)blockIdx.y * gridDim.x + blockIdx.x;
    if (t == 0) {
        unsigned *m = meta + g * PN_META;
        m[0] = (unsigned)nbytes + (first ? 2u : 0u);
        m[1] = sh_adler[0] % PN_ADLER;
        m[2] = sh_adler[1] % PN_ADLER;
        m[3] = ~sh_crc;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(blocks + g * PN_ROOM);
    for (int i = t; i < (nbytes + 15) / 16; i += PN_T) dst[i] = reinterpret_cast<const uint4 *>(obuf)[i];
}

// the exclusive scan of v over the PN_PT threads; all: the sum
__device__ __forceinline__ unsigned png_scan256(unsigned v, unsigned *wsum, unsigned &all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    all = 0;
    for (int k = 0; k < PN_PT / 64; ++k) {
        if (k < wave) before += wsum[k];
        all += wsum[k];
    }
    return before + inc - v;
}

// grid n.  off[span]: the chunk's offset in its file; tail[image]: Adler-32, the last chunk's CRC,
// its offset; sizes[image]: the file's length.  frame: the bytes a chunk adds to its payload (12 or 0)
__global__ void __launch_bounds__(PN_PT)
k_png_scan(int spans, long len, int frame, int header_bytes, const unsigned *__restrict__ meta, unsigned *__restrict__ off,
           unsigned *__restrict__ tail, int *__restrict__ sizes) {
    __shared__ unsigned wsum[PN_PT / 64];
    const int t = threadIdx.x;
    const unsigned *m = meta + (long)blockIdx.x * spans * PN_META;
    unsigned *o = off + (long)blockIdx.x * spans;
    unsigned at = (unsigned)header_bytes, a = 1, b = 0;
    for (int base = 0; base < spans; base += PN_PT) {
        const int k = base + t;
        const bool live = k < spans;
        const unsigned bytes = live ? m[k * PN_META] + frame : 0, A = live ? m[k * PN_META + 1] : 0;
        const unsigned B = live ? m[k * PN_META + 2] : 0;
        const unsigned n = live ? (unsigned)min((long)PN_SPAN, len - (long)k * PN_SPAN) : 0;
        unsigned all;
        const unsigned ahead = png_scan256(bytes, wsum, all);
        if (live) o[k] = at + ahead;
        at += all;
        const unsigned a_before = (a + png_scan256(A, wsum, all)) % PN_ADLER;
        a = (a + all) % PN_ADLER;
        png_scan256((B + n * a_before) % PN_ADLER, wsum, all);   // n a_before < 2^15 2^16
        b = (b + all) % PN_ADLER;
    }
    if (t == 0) {
        const unsigned adler = (b << 16) | a;
        const unsigned char body[13] = {'I', 'D', 'A', 'T', 1, 0, 0, 0xff, 0xff, (unsigned char)(adler >> 24),
                                        (unsigned char)(adler >> 16), (unsigned char)(adler >> 8), (unsigned char)adler};
        unsigned reg = 0xffffffffu;
        for (int i = 0; i < 13; ++i) reg = crc_byte(reg, body[i]);
        unsigned *tl = tail + blockIdx.x * 4;
        tl[0] = adler;
        tl[1] = ~reg;
        tl[2] = at;
        sizes[blockIdx.x] = (int)(at + (spans ? 0 : 2) + 9 + 2 * frame);   // framed: the chunk's 12 and IEND's 12
    }
}

__device__ __forceinline__ void png_be32(unsigned char *p, unsigned v) {
    p[0] = (unsigned char)(v >> 24);
    p[1] = (unsigned char)(v >> 16);
    p[2] = (unsigned char)(v >> 8);
    p[3] = (unsigned char)v;
}

// grid (spans + 1, n): workgroup s < spans writes chunk s, the last one everything around the chunks
__global__ void __launch_bounds__(PN_PT)
k_png_pack(int spans, int frame, PngHeader H, int header_bytes, const unsigned char *__restrict__ blocks,
           const unsigned *__restrict__ meta, const unsigned *__restrict__ off, const unsigned *__restrict__ tail,
           unsigned char *__restrict__ out, long out_stride) {
    const int t = threadIdx.x, s = blockIdx.x;
    unsigned char *file = out + (long)blockIdx.y * out_stride;
    if (s == spans) {
        if (t) return;
        for (int i = 0; i < header_bytes; ++i) file[i] = H.b[i];
        const unsigned *tl = tail + blockIdx.y * 4;
        unsigned char *p = file + tl[2];
        if (frame) {
            png_be32(p, 9);
            p[4] = 'I', p[5] = 'D', p[6] = 'A', p[7] = 'T';
            p += 8;
        }
        if (!spans) *p++ = 0x78, *p++ = 0x01;
        p[0] = 1, p[1] = 0, p[2] = 0, p[3] = 0xff, p[4] = 0xff;
        png_be32(p + 5, tl[0]);
        if (frame) {
            png_be32(p + 9, tl[1]);
            png_be32(p + 13, 0);
            p[17] = 'I', p[18] = 'E', p[19] = 'N', p[20] = 'D';
            png_be32(p + 21, 0xae426082u);
        }
        return;
    }
    const long g = (long)blockIdx.y * spans + s;
    const unsigned *m = meta + g * PN_META;
    const unsigned char *blk = blocks + g * PN_ROOM;
    const int pay = (int)m[0], lead = s == 0 ? 2 : 0, head = frame ? 8 : 0, total = pay + frame;
    const unsigned crc = m[3];
    unsigned char *dst = file + off[g];
    // byte i of the chunk: length, "IDAT", the zlib header in the first, the block, the CRC
    auto chunk_byte = [&](int i) -> unsigned {
        if (i < head) return i < 4 ? ((unsigned)pay >> (24 - 8 * i)) & 255 : (unsigned)"IDAT"[i - 4];
        i -= head;
        if (i < lead) return i ? 0x01 : 0x78;
        if (i < pay) return blk[i - lead];
        return (crc >> (24 - 8 * (i - pay))) & 255;
    };
    const int skew = (int)(reinterpret_cast<uintptr_t>(dst) & 3);
    for (int i = 4 * t - skew; i < total; i += 4 * PN_PT) {   // dst + i: a multiple of 4
        if (i >= 0 && i + 4 <= total) {
            *reinterpret_cast<unsigned *>(dst + i) =
                chunk_byte(i) | (chunk_byte(i + 1) << 8) | (chunk_byte(i + 2) << 16) | (chunk_byte(i + 3) << 24);
        } else {
            for (int k = max(i, 0); k < min(i + 4, total); ++k) dst[k] = (unsigned char)chunk_byte(k);
        }
    }
}

struct PngPlan {
    int spans;           // of one stream
    size_t blocks, meta, off, tail;   // byte offsets in the deflate workspace
    size_t ws_bytes, out_stride;
};

// n streams of len bytes; frame 12 (PNG chunks after header_bytes, IEND) or 0 (a zlib stream)
static int png_plan(const char *name, int n, long long len, int frame, int header_bytes, PngPlan &P) {
    DG_ARG(n >= 0 && n <= 65535, "%s: bad shape: n %d", name, n);
    DG_ARG(len >= 0 && len <= (1LL << 31) - (1LL << 22), "%s: bad shape: a stream of %lld bytes, at most 2^31 - 2^22", name,
           len);
    P.spans = (int)((len + PN_SPAN - 1) / PN_SPAN);
    const size_t total = (size_t)n * P.spans;
    P.blocks = 0;
    P.meta = P.blocks + total * PN_ROOM;
    P.off = P.meta + total * PN_META * 4;
    P.tail = (P.off + total * 4 + 15) / 16 * 16;
    P.ws_bytes = P.tail + (size_t)n * 16;
    // every block stored, the zlib header, the last chunk, IEND
    const size_t most = (size_t)header_bytes + (size_t)len + (size_t)P.spans * (5 + frame) + 2 + 9 + 2 * frame;
    DG_ARG(most <= 0x7fffffffu, "%s: bad shape: files of up to %zu bytes", name, most);
    P.out_stride = (most + 15) / 16 * 16;
    return DG_OK;
}

static int png_deflate_launch(const char *name, int n, long len, const unsigned char *data, long stride, int frame,
                              const PngHeader &H, int header_bytes, const PngPlan &P, unsigned char *ws, unsigned char *out,
                              size_t out_stride, int *sizes, hipStream_t s) {
    unsigned char *blocks = ws + P.blocks;
    unsigned *meta = (unsigned *)(ws + P.meta), *off = (unsigned *)(ws + P.off), *tail = (unsigned *)(ws + P.tail);
    if (P.spans) {
        hipLaunchKernelGGL(k_png_block, dim3(P.spans, n), dim3(PN_T), 0, s, data, len, stride, frame != 0, blocks, meta);
        DG_LAUNCHED(name);
    }
    hipLaunchKernelGGL(k_png_scan, dim3(n), dim3(PN_PT), 0, s, P.spans, len, frame, header_bytes, (const unsigned *)meta, off,
                       tail, sizes);
    DG_LAUNCHED(name);
    hipLaunchKernelGGL(k_png_pack, dim3(P.spans + 1, n), dim3(PN_PT), 0, s, P.spans, frame, H, header_bytes,
                       (const unsigned char *)blocks, (const unsigned *)meta, (const unsigned *)off, (const unsigned *)tail,
                       out, (long)out_stride);
    DG_LAUNCHED(name);
    return DG_OK;
}

static int png_shape(const char *name, int n, int h, int w, long long &len, long long &filt_stride) {
    DG_ARG(n >= 0 && h >= 1 && w >= 1, "%s: bad shape: n %d h %d w %d", name, n, h, w);
    DG_ARG(h <= 65535 && w <= 65535, "%s: bad shape: a frame of at most 65535 rows and columns, got %dx%d", name, h, w);
    len = (long long)h * (3LL * w + 1);
    filt_stride = (len + 15) / 16 * 16;
    return DG_OK;
}

}  // namespace dg

int dg_png_deflate_bytes(int n, long long len, size_t *ws_bytes, size_t *out_stride) {
    dg::PngPlan P;
    DG_ARG(ws_bytes && out_stride, "png_deflate_bytes: NULL result");
    if (int rc = dg::png_plan("png_deflate_bytes", n, len, 0, 0, P)) return rc;
    *ws_bytes = P.ws_bytes;
    *out_stride = P.out_stride;
    return DG_OK;
}

int dg_png_deflate(int n, long long len, const unsigned char *data, void *ws, size_t ws_bytes, unsigned char *out,
                   size_t out_stride, int *sizes, dg_stream_t stream) {
    using namespace dg;
    PngPlan P;
    if (int rc = png_plan("png_deflate", n, len, 0, 0, P)) return rc;
    if (n == 0) return DG_OK;
    DG_ARG((data || len == 0) && ws && out && sizes, "png_deflate: NULL tensor");
    DG_ARG(ws_bytes >= P.ws_bytes, "png_deflate: workspace of %zu bytes, %zu needed", ws_bytes, P.ws_bytes);
    DG_ARG(out_stride >= P.out_stride, "png_deflate: %zu bytes per stream, %zu needed", out_stride, P.out_stride);
    DG_ARG((((uintptr_t)ws) & 15) == 0 && (((uintptr_t)sizes) & 3) == 0,
           "png_deflate: the workspace must be 16-byte aligned, sizes 4-byte aligned");
    PngHeader H = {};
    return png_deflate_launch("png_deflate", n, (long)len, data, (long)len, 0, H, 0, P, (unsigned char *)ws, out, out_stride,
                              sizes, (hipStream_t)stream);
}

int dg_png_encode_bytes(int n, int h, int w, size_t *ws_bytes, size_t *out_stride) {
    dg::PngPlan P;
    long long len, fs;
    DG_ARG(ws_bytes && out_stride, "png_encode_bytes: NULL result");
    if (int rc = dg::png_shape("png_encode_bytes", n, h, w, len, fs)) return rc;
    if (int rc = dg::png_plan("png_encode_bytes", n, len, 12, 33, P)) return rc;
    *ws_bytes = (size_t)n * fs + P.ws_bytes;
    *out_stride = P.out_stride;
    return DG_OK;
}

int dg_png_encode(int n, int h, int w, const unsigned char *in, const unsigned char *header, int header_bytes, void *ws,
                  size_t ws_bytes, unsigned char *out, size_t out_stride, int *sizes, dg_stream_t stream) {
    using namespace dg;
    PngPlan P;
    long long len, fs;
    if (int rc = png_shape("png_encode", n, h, w, len, fs)) return rc;
    DG_ARG(header && header_bytes == 33, "png_encode: a header of %d bytes, signature and IHDR are 33", header_bytes);
    if (int rc = png_plan("png_encode", n, len, 12, header_bytes, P)) return rc;
    if (n == 0) return DG_OK;
    DG_ARG(in && ws && out && sizes, "png_encode: NULL tensor");
    DG_ARG(ws_bytes >= (size_t)n * fs + P.ws_bytes, "png_encode: workspace of %zu bytes, %zu needed", ws_bytes,
           (size_t)n * fs + P.ws_bytes);
    DG_ARG(out_stride >= P.out_stride, "png_encode: %zu bytes per file, %zu needed", out_stride, P.out_stride);
    DG_ARG((((uintptr_t)ws) & 15) == 0 && (((uintptr_t)sizes) & 3) == 0,
           "png_encode: the workspace must be 16-byte aligned, sizes 4-byte aligned");
    PngHeader H = {};
    for (int i = 0; i < header_bytes; ++i) H.b[i] = header[i];
    unsigned char *filt = (unsigned char *)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_png_filter, dim3(h, n), dim3(PN_PT), 0, s, h, w, in, filt, (long)fs);
    DG_LAUNCHED("png_encode (filter)");
    return png_deflate_launch("png_encode", n, (long)len, filt, (long)fs, 12, H, header_bytes, P, filt + (size_t)n * fs, out,
                              out_stride, sizes, s);
}
