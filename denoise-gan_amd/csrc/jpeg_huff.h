// The per-lane half of the JPEG entropy decoder (jpeg_dec.hip): the decoder state, the bit window
// and the decode of one subsequence.  Plain integer code for host and device alike.
#pragma once
#include "common.h"

namespace dg {

constexpr int JD_SUB = 128;                 // bytes of the unstuffed scan in a subsequence, one per lane
constexpr int JD_T = 256;                   // lanes of a decoder workgroup
constexpr int JD_SUB_BITS = JD_SUB * 8;
constexpr int JD_SUB_WORDS = JD_SUB / 4;    // 32: a subsequence is one row of LDS banks
constexpr int JD_WORDS = (JD_T + 1) * JD_SUB_WORDS;   // staged words: the workgroup's range and a row of spill
constexpr int JD_LUT_BITS = 9;
constexpr int JD_TAB_WORDS = 256 + 18 + 18 + 64;      // a code table (below)
constexpr int JD_SYMBOL_BITS = 31;          // most bits of a symbol: a code of 16 and 15 magnitude bits

// A code table, JD_TAB_WORDS words, built on the host (dgan/jpeg.py _device_table):
//   [0, 256)    2^9 uint16 entries by the next 9 bits: (length << 8) | symbol, 0 = a longer code
//   [256, 274)  int maxcode[18]: the largest code of every length, -1 where there is none
//   [274, 292)  int valoff[18]: valptr - mincode of every length
//   [292, 356)  the 256 symbols as bytes
// A workgroup holds the four tables DC0, DC1, AC0, AC1 of its image.

// The decoder state in front of a symbol: the bit position in the unstuffed scan, the block of
// the MCU (0..3 Y, 4 Cb, 5 Cr) and the zigzag index the symbol codes (0: the DC difference).
typedef unsigned long long jd_state;
__host__ __device__ __forceinline__ jd_state jd_pack(unsigned p, int blk, int zz) {
    return (jd_state)p | ((jd_state)blk << 32) | ((jd_state)zz << 40);
}

// Word i of the staged range.  Lane l reads row l, so row r is rotated by r banks: the lanes of
// a wave that are equally far into their subsequences hit different banks.
__host__ __device__ __forceinline__ int jd_swizzle(int i) { return (i & ~31) | ((i + (i >> 5)) & 31); }

struct JdSink {          // where the write pass puts the levels; coef == nullptr: count only
    short *coef;         // the image's [nblk][64], natural order, zeroed
    long first, nblk;    // the block the lane's first symbol belongs to, the image's blocks
    const unsigned char *natural;   // zigzag index -> row-major index
    bool short_of_bits;  // out: a symbol of a block below nblk reached past the scan's end
};

// Decode the symbols whose first bit lies in [state.p, limit) and return the state behind the
// last of them; count: the blocks they complete.  words: the staged range (first bit highest in a
// word), whose word 0 holds bit `base` of the scan; the caller guarantees base <= state.p and
// limit <= base + JD_T * JD_SUB_BITS, so every read stays below JD_WORDS.  total: the scan's
// bits; a symbol that would end behind them ends the decode at `total` and is not counted.  Every
// trip consumes at least one bit, so the loop is bounded by limit - state.p.
__host__ __device__ __forceinline__ jd_state jd_decode(const unsigned *words, unsigned base, const unsigned *tabs,
                                                       unsigned sel, jd_state in, unsigned limit, unsigned total,
                                                       int &count, JdSink &sink) {
    unsigned p = (unsigned)in;
    int blk = (int)(in >> 32) & 7, zz = (int)(in >> 40) & 63;
    if (blk > 5) blk = 0;
    count = 0;
    while (p < limit) {
        if (sink.coef && sink.first + count >= sink.nblk) break;   // the image is complete: padding follows
        const unsigned q = p - base;
        const unsigned long long two = ((unsigned long long)words[jd_swizzle((int)(q >> 5))] << 32) |
                                       words[jd_swizzle((int)(q >> 5) + 1)];
        const unsigned v = (unsigned)((two << (q & 31)) >> 32);   // the next 32 bits
        const int comp = blk < 4 ? 0 : blk - 3;
        const unsigned *T = tabs + ((zz ? 2 : 0) + ((sel >> (2 * comp + (zz ? 1 : 0))) & 1)) * JD_TAB_WORDS;
        const unsigned i9 = v >> (32 - JD_LUT_BITS);
        const unsigned e = (T[i9 >> 1] >> (16 * (i9 & 1))) & 0xffff;
        int len, sym;
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 255);
        } else {   // libjpeg's slow path: the first length whose largest code is not below the bits
            const int *maxcode = reinterpret_cast<const int *>(T + 256), *valoff = maxcode + 18;
            const unsigned code = v >> 16;
            len = JD_LUT_BITS + 1;
            while (len <= 16 && (int)(code >> (16 - len)) > maxcode[len]) ++len;
            if (len > 16) {   // no code: a damaged scan; go on behind 16 bits
                len = 16;
                sym = 0;
            } else {
                const unsigned at = (unsigned)(valoff[len] + (int)(code >> (16 - len))) & 255;
                sym = (int)((T[292 + (at >> 2)] >> (8 * (at & 3))) & 255);
            }
        }
        const int size = sym & 15, run = sym >> 4;
        if (p + len + size > total) {
            if (sink.coef) sink.short_of_bits = true;
            p = total;
            break;
        }
        int val = 0;
        if (size) {
            const unsigned m = (v << len) >> (32 - size);   // len + size <= JD_SYMBOL_BITS
            val = m < (1u << (size - 1)) ? (int)m - (1 << size) + 1 : (int)m;
        }
        p += len + size;
        int at = -1;   // the zigzag index val belongs to
        if (zz == 0) {
            at = 0;
            zz = 1;
        } else if (size == 0) {
            zz = run == 15 ? zz + 16 : 64;   // ZRL, else EOB
        } else {
            zz += run;
            at = zz < 64 ? zz : -1;
            ++zz;
        }
        if (sink.coef && at >= 0) sink.coef[(sink.first + count) * 64 + sink.natural[at]] = (short)val;
        if (zz >= 64) {
            zz = 0;
            blk = blk == 5 ? 0 : blk + 1;
            ++count;
        }
    }
    return jd_pack(p, blk, zz);
}

}  // namespace dg
