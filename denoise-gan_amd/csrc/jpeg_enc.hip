// Baseline JPEG encoder (include/dgan.h "Baseline JPEG encoder"; the definition in numpy:
// dgan/jpeg.py jpeg_encode_ref).  The front end is the round trip's (jpeg_front.h); the rest is the
// Huffman back end.  Eight launches, integers only:
//   k_jpeg_coef     a block per strip of four MCUs: the front end, then the quantised levels as
//                   int16 [n][mcu][6][64] in zigzag and scan order through LDS (a lane stores eight
//                   consecutive zigzag positions, 16 bytes); dummy luma blocks are filled in here
//   k_jpeg_len      a wave per block, a lane per zigzag index: every lane's code from the ballot
//                   of the nonzero lanes, their lengths summed over the wave
//   k_jpeg_lenscan  a workgroup per image: the exclusive scan of the block lengths (64-bit)
//   k_jpeg_zero     clears the streams
//   k_jpeg_emit     the lane codes again, ORed MSB first into the wave's LDS bit buffer, then copied
//                   to the image's stream shifted by the block's bit offset: interior dwords by
//                   plain stores, the two shared with the neighbouring blocks by atomicOr
//   k_jpeg_ffcount  0xFF bytes per 4096-byte chunk of a stream
//   k_jpeg_ffscan   a workgroup per image: the scan of the chunk counts, the file length
//   k_jpeg_pack     header, every chunk at its final position with 0x00 after 0xFF, EOI
// A stream dword holds its first bit highest, so byte b of a stream is bits 31 - 8 (b & 3) down.
#include <algorithm>
#include "jpeg_front.h"

namespace dg {

constexpr int JE_T = 256;            // threads of the entropy kernels: four waves
constexpr int JE_WB = 4;             // blocks a wave codes one after the other
constexpr int JE_BITS = 1660;        // most bits of a block: 11 + 11 + 63 * 26
constexpr int JE_BUF = 56;           // dwords of a wave's bit buffer: JE_BITS + 7 padding bits, a code's spill
constexpr int JE_CHUNK = JE_T * 16;  // stream bytes per workgroup of the stuffing kernels
constexpr int JE_HDR = 640;          // most header bytes (623 are written today)
constexpr int JE_ST = 1024;          // threads of k_jpeg_lenscan, eight lengths each

__constant__ unsigned char c_zigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47,
    55, 62, 63};

// Annex K.3 - K.6: codes per length 1..16 of DC0, AC0, DC1, AC1; the DC symbols are 0..11
constexpr unsigned char JH_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                          {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                          {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                          {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char JH_AC[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// every symbol's code packed (length << 16) | code, 0 where a table has none; [0] luma, [1] chroma
struct JpegHuff {
    unsigned dc[2][16];
    unsigned ac[2][256];
};
constexpr int JE_HUFF = sizeof(JpegHuff) / 4;

// Annex C: codes count up within a length and double at every longer one
constexpr JpegHuff jpeg_make_huff() {
    JpegHuff H{};
    for (int k = 0; k < 4; ++k) {
        unsigned code = 0;
        int i = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < JH_BITS[k][len - 1]; ++j, ++i, ++code) {
                const unsigned e = ((unsigned)len << 16) | code;
                if (k & 1) H.ac[k >> 1][JH_AC[k >> 1][i]] = e;
                else H.dc[k >> 1][i] = e;
            }
            code <<= 1;
        }
    }
    return H;
}
__constant__ JpegHuff c_huff = jpeg_make_huff();

struct JpegEnc {
    int mx, my;     // MCUs along w and h
    int bx8, by8;   // luma blocks inside the plane of multiples of 8
    long nblk;      // blocks of one image: mx * my * 6
    long total;     // blocks of the batch
};

struct JpegHeader {
    unsigned char b[JE_HDR];
};

__device__ __forceinline__ unsigned wave_scan(unsigned v) {   // inclusive, over the 64 lanes
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// grid (strips along w, strips along h, n)
__global__ void __launch_bounds__(JT)
k_jpeg_coef(JpegArgs A, JpegTables Q, JpegEnc E, const unsigned char *__restrict__ in, short *__restrict__ coef) {
    __shared__ int buf[JT * JLD];
    __shared__ int qt[128];
    const int t = threadIdx.x;
    const int X0 = blockIdx.x * JSW, Y0 = blockIdx.y * JSH;
    const unsigned char *img = in + (long)blockIdx.z * A.h * A.w * 3;
    int d[8], tq[8];
    jpeg_front(A, Q, img, X0, Y0, buf, qt, d, tq);
    const int b = t >> 3, c = t & 7;
    int *col = buf + b * 8 * JLD + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k * JLD] = d[k];
    __syncthreads();

    // this lane: zigzag positions p0 .. p0 + 7 of block b, which is block `idx` of the strip's MCU m
    int m, idx;
    if (b < 16) {
        m = (b & 7) >> 1;
        idx = (b >> 3) * 2 + (b & 1);
    } else {
        m = (b - 16) & 3;
        idx = 4 + ((b - 16) >> 2);
    }
    const int gmx = blockIdx.x * 4 + m;
    if (gmx >= E.mx) return;   // the strip reaches past the last MCU
    // a luma block right of or below the plane of multiples of 8 is a dummy: no AC, the DC of the
    // block before it in the MCU (itself a dummy or not); i: the real block that DC comes from
    int i = idx;
    if (idx < 4) {
        const bool right = 2 * gmx + 1 >= E.bx8, below = 2 * (int)blockIdx.y + 1 >= E.by8;
        while (i > 0 && (((i & 1) && right) || ((i >> 1) && below))) --i;
    }
    const bool dummy = i != idx;
    const int src = idx < 4 ? (i >> 1) * 8 + m * 2 + (i & 1) : b;
    const int p0 = c * 8;
    unsigned short v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int nat = c_zigzag[p0 + j];
        const int q = buf[(src * 8 + (nat >> 3)) * JLD + (nat & 7)];
        v[j] = (unsigned short)(dummy && p0 + j > 0 ? 0 : q);
    }
    uint4 o;
    o.x = v[0] | ((unsigned)v[1] << 16);
    o.y = v[2] | ((unsigned)v[3] << 16);
    o.z = v[4] | ((unsigned)v[5] << 16);
    o.w = v[6] | ((unsigned)v[7] << 16);
    const long blk = ((long)blockIdx.z * E.my * E.mx + (long)blockIdx.y * E.mx + gmx) * 6 + idx;
    *reinterpret_cast<uint4 *>(coef + blk * 64 + p0) = o;
}

// What lane k of a block's wave puts into the stream: v its coefficient (lane 0: the DC difference),
// nz the ballot of the nonzero lanes.  Lane 0 the DC code; a nonzero AC lane run >> 4 ZRL codes, the
// (run & 15, size) code and the magnitude bits, at most 3 * 11 + 16 + 10 = 59 bits; lane 63 EOB when
// its coefficient is 0; every other lane nothing.
__device__ __forceinline__ int jpeg_lane_code(int k, int v, unsigned long long nz, const unsigned *hdc,
                                              const unsigned *hac, unsigned long long &val) {
    const int size = 32 - __clz(abs(v));
    const unsigned mag = (unsigned)(v < 0 ? v + (1 << size) - 1 : v);
    val = 0;
    if (k == 0) {
        const unsigned cd = hdc[size & 15];
        val = ((unsigned long long)(cd & 0xffff) << size) | mag;
        return (int)(cd >> 16) + size;
    }
    if (v != 0) {
        const unsigned long long lower = nz & ((1ull << k) - 1) & ~1ull;   // the nonzero AC lanes below
        const int run = lower ? k - 1 - (63 - __clzll(lower)) : k - 1;
        const unsigned z = hac[0xf0], cd = hac[(((run & 15) << 4) | size) & 255];
        int len = 0;
        for (int r = 0; r < (run >> 4); ++r) {
            val = (val << (z >> 16)) | (z & 0xffff);
            len += z >> 16;
        }
        val = (((val << (cd >> 16)) | (cd & 0xffff)) << size) | mag;
        return len + (int)(cd >> 16) + size;
    }
    if (k == 63) {
        val = hac[0] & 0xffff;
        return hac[0] >> 16;
    }
    return 0;
}

// Block g of the batch: lane `lane`'s coefficient, the DC lane's as the difference to the block
// before of the same component in scan order (0 before an image's first); returns the code length
__device__ __forceinline__ int jpeg_block_code(const JpegEnc &E, const short *__restrict__ coef, long g, int lane,
                                               const JpegHuff *H, unsigned long long &val) {
    const long bi = g % E.nblk;   // in the image
    const int idx = (int)(bi % 6);
    int v = coef[g * 64 + lane];
    const int back = idx == 0 ? 3 : idx < 4 ? 1 : 6;   // Y(0,0): the MCU before's Y(1,1); chroma: its own kind
    if (lane == 0 && bi >= back) v -= coef[(g - back) * 64];
    const unsigned long long nz = __ballot(v != 0);
    const int cls = idx >= 4;
    return jpeg_lane_code(lane, v, nz, H->dc[cls], H->ac[cls], val);
}

__device__ __forceinline__ void jpeg_load_huff(unsigned *dst) {
    const unsigned *src = reinterpret_cast<const unsigned *>(&c_huff);
    for (int i = threadIdx.x; i < JE_HUFF; i += JE_T) dst[i] = src[i];
    __syncthreads();
}

// grid: ceil(total / (4 waves * JE_WB))
__global__ void __launch_bounds__(JE_T)
k_jpeg_len(JpegEnc E, const short *__restrict__ coef, unsigned *__restrict__ blen) {
    __shared__ unsigned huff[JE_HUFF];
    jpeg_load_huff(huff);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = 0; i < JE_WB; ++i) {
        const long g = ((long)blockIdx.x * (JE_T / 64) + wave) * JE_WB + i;
        if (g >= E.total) break;   // (the same for the whole wave)
        unsigned long long val;
        const unsigned len = jpeg_block_code(E, coef, g, lane, reinterpret_cast<const JpegHuff *>(huff), val);
        const unsigned sum = wave_scan(len);
        if (lane == 63) blen[g] = sum;
    }
}

// grid n: boff[i] = the bits of the image's blocks before block i, bits[image] = their total
__global__ void __launch_bounds__(JE_ST)
k_jpeg_lenscan(JpegEnc E, const unsigned *__restrict__ blen, unsigned long long *__restrict__ boff,
               long long *__restrict__ bits) {
    __shared__ unsigned wsum[JE_ST / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned *src = blen + (long)blockIdx.x * E.nblk;
    unsigned long long *dst = boff + (long)blockIdx.x * E.nblk;
    unsigned long long carry = 0;
    for (long base = 0; base < E.nblk; base += JE_ST * 8) {
        const long i0 = base + t * 8;
        unsigned v[8], s = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = i0 + j < E.nblk ? src[i0 + j] : 0;
            s += v[j];
        }
        const unsigned inc = wave_scan(s);   // 8192 blocks of at most 1660 bits: 32 bits hold it
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int k = 0; k < JE_ST / 64; ++k) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        unsigned long long run = carry + before + inc - s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (i0 + j < E.nblk) dst[i0 + j] = run;
            run += v[j];
        }
        carry += all;
        __syncthreads();
    }
    if (t == 0) bits[blockIdx.x] = (long long)carry;
}

__global__ void __launch_bounds__(JE_T)
k_jpeg_zero(uint4 *__restrict__ p, long count) {
    for (long i = (long)blockIdx.x * JE_T + threadIdx.x; i < count; i += (long)gridDim.x * JE_T)
        p[i] = make_uint4(0, 0, 0, 0);
}

// `len` bits of val, the first highest, into the bit buffer at bit `pos` (len <= 64; three dwords)
__device__ __forceinline__ void jpeg_put_bits(unsigned *bb, int pos, unsigned long long val, int len) {
    const unsigned long long v = val << (64 - len);
    const int s = pos & 31;
    unsigned *d = bb + (pos >> 5);
    atomicOr(d, (unsigned)(v >> 32) >> s);
    atomicOr(d + 1, (unsigned)(v >> s));
    if (s) atomicOr(d + 2, (unsigned)v << (32 - s));
}

// grid as k_jpeg_len.  stream: n x stride dwords, zero; an image whose bits exceed cap_bits is left out
__global__ void __launch_bounds__(JE_T)
k_jpeg_emit(JpegEnc E, const short *__restrict__ coef, const unsigned long long *__restrict__ boff,
            const long long *__restrict__ bits, long long cap_bits, unsigned *__restrict__ stream, long stride) {
    __shared__ unsigned huff[JE_HUFF];
    __shared__ unsigned bbuf[JE_T / 64][JE_BUF];
    jpeg_load_huff(huff);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *bb = bbuf[wave];
    for (int i = 0; i < JE_WB; ++i) {   // every wave makes every trip: the barriers below
        const long g = ((long)blockIdx.x * (JE_T / 64) + wave) * JE_WB + i;
        const bool live = g < E.total;
        if (lane < JE_BUF) bb[lane] = 0;
        __syncthreads();
        unsigned long long val = 0, off = 0;
        int len = 0, total = 0;
        long image = 0;
        if (live) {
            len = jpeg_block_code(E, coef, g, lane, reinterpret_cast<const JpegHuff *>(huff), val);
            const int end = (int)wave_scan((unsigned)len);
            total = __shfl(end, 63);
            if (len) jpeg_put_bits(bb, end - len, val, len);
            image = g / E.nblk;
            off = boff[g];
            if (g % E.nblk == E.nblk - 1) {   // the image's last block: 1 bits up to the byte
                const int pad = (int)((0 - (off + total)) & 7);
                if (lane == 0 && pad) jpeg_put_bits(bb, total, (1u << pad) - 1, pad);
                total += pad;
            }
        }
        __syncthreads();
        const int s = (int)(off & 31);
        const int nd = (s + total + 31) >> 5;   // stream dwords the block touches: at most 53
        const long d0 = (long)(off >> 5);
        const long long have = live ? bits[image] : 0;
        if (live && have <= cap_bits && d0 + nd <= stride && lane < nd) {
            const unsigned hi = lane ? bb[lane - 1] : 0, lo = bb[lane];
            const unsigned word = s ? (hi << (32 - s)) | (lo >> s) : lo;
            unsigned *dst = stream + image * stride + d0 + lane;
            if (lane == 0 || lane == nd - 1) atomicOr(dst, word);
            else *dst = word;
        }
        __syncthreads();
    }
}

// the 0xFF bytes among a thread's 16 stream bytes [b0, b0 + 16) below `ub`; q: the four dwords
__device__ __forceinline__ int jpeg_ff16(const unsigned *__restrict__ stream, long stride, long b0, long ub, uint4 &q) {
    q = make_uint4(0, 0, 0, 0);
    if (b0 >= ub || b0 + 16 > stride * 4) return 0;
    q = *reinterpret_cast<const uint4 *>(stream + b0 / 4);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        cnt += (b0 + k < ub) && ((w[k >> 2] >> (24 - 8 * (k & 3))) & 255) == 255;
    return cnt;
}

__device__ __forceinline__ long jpeg_stream_bytes(long long bits, long long cap_bits) {
    return bits >= 0 && bits <= cap_bits ? (long)((bits + 7) >> 3) : 0;
}

// grid (chunks, n)
__global__ void __launch_bounds__(JE_T)
k_jpeg_ffcount(const unsigned *__restrict__ stream, long stride, const long long *__restrict__ bits, long long cap_bits,
               unsigned *__restrict__ cnt) {
    __shared__ unsigned wsum[JE_T / 64];
    const long ub = jpeg_stream_bytes(bits[blockIdx.y], cap_bits);
    uint4 q;
    const unsigned c = jpeg_ff16(stream + (long)blockIdx.y * stride, stride,
                                 (long)blockIdx.x * JE_CHUNK + threadIdx.x * 16, ub, q);
    const unsigned inc = wave_scan(c);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0) cnt[(long)blockIdx.y * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// grid n: cnt[image][chunk] -> the 0xFF bytes before the chunk; sizes[image] = the file's length
__global__ void __launch_bounds__(JE_T)
k_jpeg_ffscan(unsigned *__restrict__ cnt, int nchunk, const long long *__restrict__ bits, long long cap_bits,
              int header_bytes, unsigned *__restrict__ fftot, int *__restrict__ sizes) {
    __shared__ unsigned wsum[JE_T / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned *c = cnt + (long)blockIdx.x * nchunk;
    unsigned carry = 0;
    for (int base = 0; base < nchunk; base += JE_T) {
        const unsigned v = base + t < nchunk ? c[base + t] : 0;
        const unsigned inc = wave_scan(v);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int k = 0; k < JE_T / 64; ++k) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        if (base + t < nchunk) c[base + t] = carry + before + inc - v;
        carry += all;
        __syncthreads();
    }
    if (t == 0) {
        const long long b = bits[blockIdx.x];
        fftot[blockIdx.x] = carry;
        sizes[blockIdx.x] = b >= 0 && b <= cap_bits ? (int)(header_bytes + jpeg_stream_bytes(b, cap_bits) + carry + 2) : -1;
    }
}

// grid (chunks, n): out + image * out_stride = header, stuffed stream, EOI
__global__ void __launch_bounds__(JE_T)
k_jpeg_pack(JpegHeader H, int header_bytes, const unsigned *__restrict__ stream, long stride,
            const long long *__restrict__ bits, long long cap_bits, const unsigned *__restrict__ cnt,
            const unsigned *__restrict__ fftot, unsigned char *__restrict__ out, long out_stride) {
    __shared__ unsigned wsum[JE_T / 64];
    const long long have = bits[blockIdx.y];
    if (have < 0 || have > cap_bits) return;   // (the whole workgroup)
    const long ub = jpeg_stream_bytes(have, cap_bits);
    const int t = threadIdx.x;
    const long b0 = (long)blockIdx.x * JE_CHUNK + t * 16;
    uint4 q;
    const unsigned c = jpeg_ff16(stream + (long)blockIdx.y * stride, stride, b0, ub, q);
    const unsigned inc = wave_scan(c);
    if ((t & 63) == 63) wsum[t >> 6] = inc;
    __syncthreads();
    unsigned before = cnt[(long)blockIdx.y * gridDim.x + blockIdx.x] + inc - c;
    for (int k = 0; k < (t >> 6); ++k) before += wsum[k];
    unsigned char *file = out + (long)blockIdx.y * out_stride;
    // header_bytes + ub + fftot + 2 <= header_bytes + 8 * stride + 2 <= out_stride (the host checks)
    if (b0 < ub && b0 + 16 <= stride * 4) {
        unsigned char *dst = file + header_bytes + b0 + before;
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        const int m = (int)min(16L, ub - b0);
        for (int k = 0; k < m; ++k) {
            const unsigned char v = (unsigned char)(w[k >> 2] >> (24 - 8 * (k & 3)));
            *dst++ = v;
            if (v == 255) *dst++ = 0;
        }
    }
    if (blockIdx.x == 0) {
        for (int k = t; k < header_bytes; k += JE_T) file[k] = H.b[k];
        if (t == 0) {
            unsigned char *eoi = file + header_bytes + ub + fftot[blockIdx.y];
            eoi[0] = 0xff;
            eoi[1] = 0xd9;
        }
    }
}

static int jpeg_enc_shape(const char *name, int n, int h, int w, JpegArgs &A, JpegEnc &E) {
    if (int rc = jpeg_shape(name, n, h, w, A)) return rc;
    DG_ARG(h <= 65535 && w <= 65535, "%s: bad shape: a JPEG file holds 1..65535 rows and columns, got %dx%d", name, h, w);
    E.mx = (w + 15) / 16;
    E.my = (h + 15) / 16;
    E.bx8 = (w + 7) / 8;
    E.by8 = (h + 7) / 8;
    E.nblk = (long)E.mx * E.my * 6;
    E.total = E.nblk * n;
    DG_ARG(E.total <= (1L << 30), "%s: bad shape: %ld blocks in one call, at most 2^30", name, E.total);
    return DG_OK;
}

// the workspace: coefficients, block offsets, block lengths
static size_t jpeg_enc_ws(const JpegEnc &E) { return (size_t)E.total * (128 + 8 + 4); }

struct JpegOut {
    long stride;   // dwords of one stream: a multiple of 4
    int nchunk;
    size_t stream_bytes, out_stride;
};

static int jpeg_enc_out(const char *name, int n, long long max_bits, int header_bytes, JpegOut &O) {
    DG_ARG(n >= 0 && n <= 65535, "%s: bad shape: n %d", name, n);
    DG_ARG(max_bits >= 0 && max_bits <= (1LL << 30) * (JE_BITS + 7), "%s: max_bits %lld out of range", name, max_bits);
    DG_ARG(header_bytes >= 0 && header_bytes <= JE_HDR, "%s: header of %d bytes, at most %d", name, header_bytes, JE_HDR);
    O.stride = (long)((max_bits / 32 + 2 + 3) / 4 * 4);
    const long chunks = (O.stride * 4 + JE_CHUNK - 1) / JE_CHUNK;
    DG_ARG(chunks <= 65535 * 1024L, "%s: max_bits %lld out of range", name, max_bits);
    O.nchunk = (int)chunks;
    // streams, then per image the chunk counts and the count of all 0xFF bytes
    O.stream_bytes = (size_t)n * ((size_t)O.stride * 4 + (size_t)O.nchunk * 4 + 4);
    O.out_stride = ((size_t)header_bytes + 8 * (size_t)O.stride + 2 + 3) / 4 * 4;
    return DG_OK;
}

}  // namespace dg

int dg_jpeg_encode_ws_bytes(int n, int h, int w, size_t *bytes) {
    dg::JpegArgs A;
    dg::JpegEnc E;
    DG_ARG(bytes, "jpeg_encode_ws_bytes: NULL result");
    if (int rc = dg::jpeg_enc_shape("jpeg_encode_ws_bytes", n, h, w, A, E)) return rc;
    *bytes = dg::jpeg_enc_ws(E);
    return DG_OK;
}

int dg_jpeg_encode_scan(int n, int h, int w, const unsigned char *in, const unsigned char *qtab, void *ws,
                        size_t ws_bytes, long long *bits, dg_stream_t stream) {
    using namespace dg;
    JpegArgs A;
    JpegEnc E;
    if (int rc = jpeg_enc_shape("jpeg_encode_scan", n, h, w, A, E)) return rc;
    DG_ARG(qtab, "jpeg_encode_scan: NULL quantisation tables");
    JpegTables Q;
    for (int i = 0; i < 128; ++i) {
        DG_ARG(qtab[i] >= 1, "jpeg_encode_scan: quantisation table entry %d is 0", i);
        Q.t[i] = qtab[i];
    }
    if (n == 0) return DG_OK;
    DG_ARG(in && ws && bits, "jpeg_encode_scan: NULL tensor");
    DG_ARG(ws_bytes >= jpeg_enc_ws(E), "jpeg_encode_scan: workspace of %zu bytes, %zu needed", ws_bytes, jpeg_enc_ws(E));
    DG_ARG((((uintptr_t)ws) & 15) == 0 && (((uintptr_t)bits) & 7) == 0,
           "jpeg_encode_scan: the workspace must be 16-byte aligned, bits 8-byte aligned");
    short *coef = (short *)ws;
    unsigned long long *boff = (unsigned long long *)(coef + E.total * 64);
    unsigned *blen = (unsigned *)(boff + E.total);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_jpeg_coef, dim3(A.Wp / JSW, A.Hp / JSH, n), dim3(JT), 0, s, A, Q, E, in, coef);
    DG_LAUNCHED("jpeg_encode_scan (coefficients)");
    hipLaunchKernelGGL(k_jpeg_len, dim3(dg_cdiv(E.total, JE_T / 64 * JE_WB)), dim3(JE_T), 0, s, E, (const short *)coef,
                       blen);
    DG_LAUNCHED("jpeg_encode_scan (lengths)");
    hipLaunchKernelGGL(k_jpeg_lenscan, dim3(n), dim3(JE_ST), 0, s, E, (const unsigned *)blen, boff, bits);
    DG_LAUNCHED("jpeg_encode_scan (scan)");
    return DG_OK;
}

int dg_jpeg_encode_out_bytes(int n, long long max_bits, int header_bytes, size_t *stream_bytes, size_t *out_stride) {
    dg::JpegOut O;
    DG_ARG(stream_bytes && out_stride, "jpeg_encode_out_bytes: NULL result");
    if (int rc = dg::jpeg_enc_out("jpeg_encode_out_bytes", n, max_bits, header_bytes, O)) return rc;
    *stream_bytes = O.stream_bytes;
    *out_stride = O.out_stride;
    return DG_OK;
}

int dg_jpeg_encode_emit(int n, int h, int w, const void *ws, size_t ws_bytes, const long long *bits, long long max_bits,
                        const unsigned char *header, int header_bytes, void *stream_ws, size_t stream_bytes,
                        unsigned char *out, size_t out_stride, int *sizes, dg_stream_t stream) {
    using namespace dg;
    JpegArgs A;
    JpegEnc E;
    JpegOut O;
    if (int rc = jpeg_enc_shape("jpeg_encode_emit", n, h, w, A, E)) return rc;
    if (int rc = jpeg_enc_out("jpeg_encode_emit", n, max_bits, header_bytes, O)) return rc;
    DG_ARG(max_bits <= E.nblk * (long long)JE_BITS, "jpeg_encode_emit: max_bits %lld, %ld blocks hold at most %lld",
           max_bits, E.nblk, E.nblk * (long long)JE_BITS);
    DG_ARG(header, "jpeg_encode_emit: NULL header");
    if (n == 0) return DG_OK;
    DG_ARG(ws && bits && stream_ws && out && sizes, "jpeg_encode_emit: NULL tensor");
    DG_ARG(ws_bytes >= jpeg_enc_ws(E), "jpeg_encode_emit: workspace of %zu bytes, %zu needed", ws_bytes, jpeg_enc_ws(E));
    DG_ARG(stream_bytes >= O.stream_bytes, "jpeg_encode_emit: stream workspace of %zu bytes, %zu needed", stream_bytes,
           O.stream_bytes);
    DG_ARG(out_stride >= O.out_stride, "jpeg_encode_emit: %zu bytes per file, %zu needed", out_stride, O.out_stride);
    DG_ARG((((uintptr_t)ws) & 15) == 0 && (((uintptr_t)stream_ws) & 15) == 0 && (((uintptr_t)bits) & 7) == 0 &&
               (((uintptr_t)sizes) & 3) == 0,
           "jpeg_encode_emit: the workspaces must be 16-byte aligned, bits 8-byte and sizes 4-byte aligned");
    JpegHeader H;
    for (int i = 0; i < JE_HDR; ++i) H.b[i] = i < header_bytes ? header[i] : 0;
    const short *coef = (const short *)ws;
    const unsigned long long *boff = (const unsigned long long *)(coef + E.total * 64);
    unsigned *str = (unsigned *)stream_ws;
    unsigned *cnt = str + (size_t)n * O.stride;
    unsigned *fftot = cnt + (size_t)n * O.nchunk;
    hipStream_t s = (hipStream_t)stream;
    const long quads = (long)n * O.stride / 4;
    hipLaunchKernelGGL(k_jpeg_zero, dim3((unsigned)std::min<long>(dg_cdiv(quads, JE_T), 4096)), dim3(JE_T), 0, s,
                       (uint4 *)str, quads);
    DG_LAUNCHED("jpeg_encode_emit (zero)");
    hipLaunchKernelGGL(k_jpeg_emit, dim3(dg_cdiv(E.total, JE_T / 64 * JE_WB)), dim3(JE_T), 0, s, E, coef, boff, bits,
                       max_bits, str, O.stride);
    DG_LAUNCHED("jpeg_encode_emit (codes)");
    hipLaunchKernelGGL(k_jpeg_ffcount, dim3(O.nchunk, n), dim3(JE_T), 0, s, (const unsigned *)str, O.stride, bits,
                       max_bits, cnt);
    DG_LAUNCHED("jpeg_encode_emit (count)");
    hipLaunchKernelGGL(k_jpeg_ffscan, dim3(n), dim3(JE_T), 0, s, cnt, O.nchunk, bits, max_bits, header_bytes, fftot,
                       sizes);
    DG_LAUNCHED("jpeg_encode_emit (scan)");
    hipLaunchKernelGGL(k_jpeg_pack, dim3(O.nchunk, n), dim3(JE_T), 0, s, H, header_bytes, (const unsigned *)str,
                       O.stride, bits, max_bits, (const unsigned *)cnt, (const unsigned *)fftot, out, (long)out_stride);
    DG_LAUNCHED("jpeg_encode_emit (pack)");
    return DG_OK;
}
