// phc_jpeg.h -- per-block / per-segment code of phc_jpeg_encode (csrc/phc_jpeg.hip; contract and the coding rules: include/phc_amd.h): baseline JPEG scans of F
// device frames, so that a recorded frame leaves the device compressed.
// PHC_HD: tests/jpeg_shim.cpp and tests/jpeg_asan_main.cpp build everything here for the CPU and run the launch as plain loops over blocks and segments.
//
// The launch is four passes over one scratch block (jpeg_layout):
//   1 jpeg_block      one lane per 8 x 8 block of a component plane: fetch (edge replication, 2 x 2 chroma mean), colour, DCT, quantiser, zigzag -> coef
//   2 jpeg_segment    one lane per restart segment: Huffman-code its MCUs into the segment's slot of worst-case size, pad, append RSTn -> seg_len
//   3 (scan)          one workgroup per frame: exclusive sum of the segment lengths -> seg_off, the frame's length
//   4 jpeg_copy_segment  one wavefront per segment: its bytes from the slot to their place in the frame's contiguous run
// Everything a lane indexes with a run-time value lives in memory (coef, the Huffman table, the slot); the 64 samples of a block and the bit accumulator are
// indexed by unrolled loops only and stay in registers.
//
// Worst case of a block, in bits (the bound every buffer size rests on):
//   DC   the longest DC code is 11 bits (chrominance, category 11: Table K.4) and carries 11 extra bits: 22.  The quantiser clamps a DC value to
//        [-1024, 1023], so a difference lies in [-2047, 2047]: category <= 11 always.
//   AC   a non-zero coefficient costs at most a 16-bit code (Tables K.5 / K.6) + 10 extra bits = 26 (the quantiser clamps to [-1023, 1023]: category <= 10);
//        a zero costs less wherever it goes: a ZRL (11 / 10 bits) covers 16 positions and EOB (4 / 2 bits) appears only when position 63 is zero.  So 63
//        non-zero coefficients are the worst: 63 x 26 = 1638.
//   JPEG_BLOCK_MAX_BITS = 22 + 1638 = 1660.  (The clamps never bind on 8-bit input: |DC| <= 1024 and |AC| <= 127.5 x sum|basis| <= 1020 before the division.)
// A segment of n MCUs holds 6 n blocks: ceil(6 n x 1660 / 8) bytes including the 1-padding of its last byte, twice that if every byte were 0xFF and stuffed,
// plus the 2 bytes of its RSTn marker: jpeg_slot_bytes.  A frame's bound is segments x slot (jpeg_frame_bound).
#pragma once
#include <stdint.h>
#include <math.h>
#include "phc_math.h"
#include "../../include/phc_amd.h"

namespace phc {

constexpr int JPEG_BLOCK_MAX_BITS = 22 + 63 * 26;

struct alignas(16) JpegU4 { uint32_t x, y, z, w; };   // eight coefficients: one 16-byte access

// ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------------
struct JpegGeom {
    int32_t mcux, mcuy, nmcu;   // 16 x 16 MCUs across, down, per frame
    int32_t ri;                 // MCUs per segment actually used: min(restart interval, nmcu)
    int32_t nseg;               // segments per frame
    int64_t blocks;             // 8 x 8 blocks per frame: 6 nmcu (Y plane 4 nmcu in raster order of a 2 mcux wide grid, then Cb, then Cr)
    int64_t slot_bytes;
};
PHC_HD int64_t jpeg_slot_bytes(int64_t mcus) { return 2 * ((6 * mcus * JPEG_BLOCK_MAX_BITS + 7) / 8) + 2; }
PHC_HD JpegGeom jpeg_geom(int W, int H, int restart_interval) {
    JpegGeom g;
    g.mcux = (W + 15) / 16; g.mcuy = (H + 15) / 16; g.nmcu = g.mcux * g.mcuy;
    g.ri = restart_interval < g.nmcu ? restart_interval : g.nmcu;
    g.nseg = (g.nmcu + g.ri - 1) / g.ri;
    g.blocks = 6 * (int64_t)g.nmcu;
    g.slot_bytes = jpeg_slot_bytes(g.ri);
    return g;
}
PHC_HD int64_t jpeg_frame_bound(const JpegGeom& g) { return (int64_t)g.nseg * g.slot_bytes; }

// scratch block: coefficients (used when the caller passes no `coef`), segment lengths, segment offsets, slots; every part starts on a multiple of 16 bytes
struct JpegLayout { int64_t coef, seg_len, seg_off, slots, total; };
PHC_HD int64_t jpeg_up16(int64_t v) { return (v + 15) / 16 * 16; }
PHC_HD JpegLayout jpeg_layout(const JpegGeom& g, int64_t F) {
    JpegLayout l;
    l.coef = 0;
    l.seg_len = jpeg_up16(F * g.blocks * 128);
    l.seg_off = l.seg_len + jpeg_up16(F * g.nseg * 4);
    l.slots = l.seg_off + jpeg_up16(F * g.nseg * 4);
    l.total = l.slots + jpeg_up16(F * g.nseg * g.slot_bytes);
    return l;
}

// what the kernels are handed: the caller's arrays, the parts of the scratch block and the two quantiser tables (zigzag order) by value
struct JpegK {
    JpegGeom g;
    int32_t F, W, H;
    int64_t row_stride, frame_stride, out_stride;
    const uint8_t* rgba;
    int16_t* coef;
    int32_t* seg_len;
    int32_t* seg_off;
    uint8_t* slots;
    uint8_t* out;
    int32_t* length;
    uint8_t q[2][64];
};

inline int32_t jpeg_args_check(const phc_jpeg_args_t* a) {
    if (!a || !a->rgba || !a->qtab || !a->out || !a->length || !a->scratch) return PHC_EINVAL;
    if (a->width < 1 || a->width > 65535 || a->height < 1 || a->height > 65535 || a->num_frames < 0 || a->restart_interval < 1) return PHC_EINVAL;
    for (int i = 0; i < 128; ++i) if (a->qtab[i] == 0) return PHC_EINVAL;
    if (a->row_stride < 4 * (int64_t)a->width || (a->row_stride & 3) || a->frame_stride < a->row_stride * a->height || (a->frame_stride & 3)) return PHC_EINVAL;
    if (((uintptr_t)a->rgba & 3) || ((uintptr_t)a->scratch & 15) || ((uintptr_t)a->coef & 15)) return PHC_EINVAL;
    const JpegGeom g = jpeg_geom(a->width, a->height, a->restart_interval);
    if (jpeg_frame_bound(g) > 0x7fffffffLL) return PHC_EUNSUPPORTED;   // a frame's offsets and its length are 32-bit
    if (a->out_stride < jpeg_frame_bound(g) || a->scratch_bytes < jpeg_layout(g, a->num_frames).total) return PHC_EINVAL;
    return 0;
}

inline JpegK jpeg_kargs(const phc_jpeg_args_t* a) {
    JpegK k;
    k.g = jpeg_geom(a->width, a->height, a->restart_interval);
    const JpegLayout l = jpeg_layout(k.g, a->num_frames);
    uint8_t* s = (uint8_t*)a->scratch;
    k.F = a->num_frames; k.W = a->width; k.H = a->height;
    k.row_stride = a->row_stride; k.frame_stride = a->frame_stride; k.out_stride = a->out_stride;
    k.rgba = a->rgba;
    k.coef = a->coef ? a->coef : (int16_t*)(s + l.coef);
    k.seg_len = (int32_t*)(s + l.seg_len); k.seg_off = (int32_t*)(s + l.seg_off); k.slots = s + l.slots;
    k.out = a->out; k.length = a->length;
    for (int i = 0; i < 128; ++i) k.q[i / 64][i % 64] = a->qtab[i];
    return k;
}

// ---- pass 1: one 8 x 8 block ------------------------------------------------------------------------------------------------------------------------------
// zigzag position -> row-major index 8 v + u (Figure A.6)
#define PHC_JPEG_ZIGZAG {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, \
                         15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// M[u][x] = C(u) / 2 cos((2 x + 1) u pi / 16): the orthonormal DCT-II matrix, S = M s M^T (A.3.3).  h[n] = cos(n pi / 16) / 2; the angle folds into 0 .. 8.
PHC_HD constexpr float jpeg_dct_m(int u, int x) {
    constexpr float h[9] = {0.5f, 0.49039264020161522f, 0.46193976625564337f, 0.41573480615127262f, 0.35355339059327379f, 0.27778511650980114f,
                            0.19134171618254489f, 0.097545161008064134f, 0.f};
    if (u == 0) return 0.35355339059327379f;
    int n = ((2 * x + 1) * u) % 32;
    if (n > 16) n = 32 - n;
    return n > 8 ? -h[16 - n] : h[n];
}

PHC_HD uint32_t jpeg_pixel(const JpegK& k, const uint8_t* frame, int x, int y) {   // the frame extended by its last column and row
    x = x < k.W ? x : k.W - 1;
    y = y < k.H ? y : k.H - 1;
    return *(const uint32_t*)(frame + (int64_t)y * k.row_stride + 4 * (int64_t)x);
}

// block b of frame f (b < 4 nmcu: Y; then Cb; then Cr): its 64 quantised coefficients in zigzag order -> coef[f][b][0..63]
PHC_HD void jpeg_block(const JpegK& k, int64_t f, int64_t b) {
    const uint8_t* frame = k.rgba + f * k.frame_stride;
    const int64_t ny = 4 * (int64_t)k.g.nmcu;
    const int comp = b < ny ? 0 : (b < ny + k.g.nmcu ? 1 : 2);
    float s[64];
    if (comp == 0) {
        const int bx = (int)(b % (2 * k.g.mcux)), by = (int)(b / (2 * k.g.mcux));
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const uint32_t p = jpeg_pixel(k, frame, 8 * bx + (i & 7), 8 * by + (i >> 3));
            const float r = (float)(p & 255u), g = (float)((p >> 8) & 255u), bl = (float)((p >> 16) & 255u);
            s[i] = ((0.299f * r + 0.587f * g) + 0.114f * bl) - 128.f;
        }
    } else {
        const int64_t c = b - ny - (comp == 2 ? k.g.nmcu : 0);
        const int bx = (int)(c % k.g.mcux), by = (int)(c / k.g.mcux);
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const int x = 2 * (8 * bx + (i & 7)), y = 2 * (8 * by + (i >> 3));
            const uint32_t p0 = jpeg_pixel(k, frame, x, y), p1 = jpeg_pixel(k, frame, x + 1, y), p2 = jpeg_pixel(k, frame, x, y + 1), p3 = jpeg_pixel(k, frame, x + 1, y + 1);
            // the mean of the group's R, G, B (sums of four bytes, exact), then the chroma of the mean: the mean of the four chroma values
            const float r = 0.25f * (float)((p0 & 255u) + (p1 & 255u) + (p2 & 255u) + (p3 & 255u));
            const float g = 0.25f * (float)(((p0 >> 8) & 255u) + ((p1 >> 8) & 255u) + ((p2 >> 8) & 255u) + ((p3 >> 8) & 255u));
            const float bl = 0.25f * (float)(((p0 >> 16) & 255u) + ((p1 >> 16) & 255u) + ((p2 >> 16) & 255u) + ((p3 >> 16) & 255u));
            s[i] = comp == 1 ? ((-0.168735892f * r - 0.331264108f * g) + 0.5f * bl) : ((0.5f * r - 0.418687589f * g) - 0.081312411f * bl);   // (+128 and the level shift cancel)
        }
    }
    // rows, then columns: eight-term sums in index order
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        float r[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) r[x] = s[8 * y + x];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float acc = jpeg_dct_m(u, 0) * r[0];
#pragma unroll
            for (int x = 1; x < 8; ++x) acc += jpeg_dct_m(u, x) * r[x];
            s[8 * y + u] = acc;
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float r[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) r[y] = s[8 * y + u];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            float acc = jpeg_dct_m(v, 0) * r[0];
#pragma unroll
            for (int y = 1; y < 8; ++y) acc += jpeg_dct_m(v, y) * r[y];
            s[8 * v + u] = acc;
        }
    }
    constexpr uint8_t zz[64] = PHC_JPEG_ZIGZAG;
    const uint8_t* q = k.q[comp ? 1 : 0];
    JpegU4* dst = (JpegU4*)(k.coef + (f * k.g.blocks + b) * 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int z = 8 * j + i;
            const float v = s[zz[z]];
            const int m = (int)floorf(fabsf(v) / (float)q[z] + 0.5f);
            int c = v < 0.f ? -m : m;
            const int lo = z == 0 ? -1024 : -1023;                         // (a black block at q = 1 has DC = -1024; the clamps never bind on 8-bit input
            c = c < lo ? lo : (c > 1023 ? 1023 : c);                       //  and keep every category within the Huffman tables whatever the input)
            const uint32_t h = (uint32_t)(uint16_t)(int16_t)c;
            w[i >> 1] = (i & 1) ? (w[i >> 1] | (h << 16)) : h;
        }
        JpegU4 o; o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
        dst[j] = o;
    }
}

// ---- pass 2: one restart segment ----------------------------------------------------------------------------------------------------------------------------
// Annex K.3 - K.6: BITS (codes per length 1 .. 16) and HUFFVAL; the same arrays go into the DHT segments of the header (phc_amd/video.py)
#define PHC_JPEG_DC_VALS {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}
#define PHC_JPEG_DC_LUMA_BITS {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}
#define PHC_JPEG_DC_CHROMA_BITS {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}
#define PHC_JPEG_AC_LUMA_BITS {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}
#define PHC_JPEG_AC_LUMA_VALS {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, \
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, \
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, \
    0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, \
    0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, \
    0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}
#define PHC_JPEG_AC_CHROMA_BITS {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}
#define PHC_JPEG_AC_CHROMA_VALS {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, \
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, \
    0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, \
    0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, \
    0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, \
    0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}

// symbol -> code << 5 | length (length 0: no such symbol), by the procedure of Annex C
struct JpegHuff { uint32_t dc[2][12]; uint32_t ac[2][256]; };
constexpr int JPEG_HUFF_WORDS = (int)(sizeof(JpegHuff) / 4);

template <int NV, int NSYM>
constexpr void jpeg_huff_fill(uint32_t (&tab)[NSYM], const uint8_t (&bits)[16], const uint8_t (&vals)[NV]) {
    for (int i = 0; i < NSYM; ++i) tab[i] = 0;
    uint32_t code = 0;
    int n = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) tab[vals[n++]] = (code++ << 5) | (uint32_t)len;
        code <<= 1;
    }
}
constexpr JpegHuff jpeg_huff_make() {
    constexpr uint8_t dcv[12] = PHC_JPEG_DC_VALS, dlb[16] = PHC_JPEG_DC_LUMA_BITS, dcb[16] = PHC_JPEG_DC_CHROMA_BITS;
    constexpr uint8_t alb[16] = PHC_JPEG_AC_LUMA_BITS, alv[162] = PHC_JPEG_AC_LUMA_VALS, acb[16] = PHC_JPEG_AC_CHROMA_BITS, acv[162] = PHC_JPEG_AC_CHROMA_VALS;
    JpegHuff h{};
    jpeg_huff_fill(h.dc[0], dlb, dcv);
    jpeg_huff_fill(h.dc[1], dcb, dcv);
    jpeg_huff_fill(h.ac[0], alb, alv);
    jpeg_huff_fill(h.ac[1], acb, acv);
    return h;
}

// the bit writer: the accumulator and its count are a lane's registers, the byte pointer is data-dependent.  A put is at most 27 bits on top of at most 7
// pending ones.  Every 0xFF byte is followed by 0x00 (F.1.2.3).
struct JpegBits { uint64_t acc; int n; uint8_t* p; };
PHC_HD void jpeg_put(JpegBits& w, uint32_t code, int len) {
    w.acc = (w.acc << len) | code;
    w.n += len;
    while (w.n >= 8) {
        const uint8_t b = (uint8_t)(w.acc >> (w.n - 8));
        *w.p++ = b;
        if (b == 0xff) *w.p++ = 0;
        w.n -= 8;
    }
}
PHC_HD int jpeg_category(int v) {   // SSSS: bits of |v| (F.1.2.1.2)
    const uint32_t m = (uint32_t)(v < 0 ? -v : v);
    return m ? 32 - __builtin_clz(m) : 0;
}
// a value of category s: the code of its symbol, then the s low bits of v (v > 0) or of v - 1 (v < 0)
PHC_HD void jpeg_put_value(JpegBits& w, uint32_t entry, int v, int s) {
    const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
    jpeg_put(w, ((entry >> 5) << s) | extra, (int)(entry & 31u) + s);
}

// one block: DC difference, then the AC run lengths (F.1.2.2: ZRL for runs of 16, EOB unless coefficient 63 is non-zero).  -> the block's DC value
PHC_HD int jpeg_code_block(JpegBits& w, const JpegHuff& h, int t, const JpegU4* blk, int pred) {
    int run = 0, dc = 0;
#pragma unroll 1
    for (int j = 0; j < 8; ++j) {
        const JpegU4 u = blk[j];
        if (j > 0 && (u.x | u.y | u.z | u.w) == 0u) { run += 8; continue; }
        const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int v = (int)(int16_t)(uint16_t)(wd[i >> 1] >> (16 * (i & 1)));
            if (j == 0 && i == 0) {
                dc = v;
                const int d = v - pred, s = jpeg_category(d);
                jpeg_put_value(w, h.dc[t][s], d, s);
            } else if (v == 0) {
                ++run;
            } else {
                while (run >= 16) { jpeg_put(w, h.ac[t][0xf0] >> 5, (int)(h.ac[t][0xf0] & 31u)); run -= 16; }
                const int s = jpeg_category(v);
                jpeg_put_value(w, h.ac[t][(run << 4) | s], v, s);
                run = 0;
            }
        }
    }
    if (run > 0) jpeg_put(w, h.ac[t][0] >> 5, (int)(h.ac[t][0] & 31u));
    return dc;
}

// segment sg of frame f into its slot: MCUs sg ri .. , each Y00 Y01 Y10 Y11 Cb Cr; the last byte padded with 1-bits; RST(sg mod 8) behind every segment
// but the frame's last.  -> seg_len
PHC_HD void jpeg_segment(const JpegK& k, const JpegHuff& h, int64_t f, int sg) {
    const JpegGeom& g = k.g;
    const JpegU4* coef = (const JpegU4*)(k.coef + f * g.blocks * 64);
    uint8_t* slot = k.slots + (f * g.nseg + sg) * g.slot_bytes;
    JpegBits w;
    w.acc = 0; w.n = 0; w.p = slot;
    int py = 0, pcb = 0, pcr = 0;
    const int m0 = sg * g.ri, m1 = m0 + g.ri < g.nmcu ? m0 + g.ri : g.nmcu;
    for (int m = m0; m < m1; ++m) {
        const int mx = m % g.mcux, my = m / g.mcux;
#pragma unroll 1
        for (int b = 0; b < 6; ++b) {
            int64_t idx;
            if (b < 4) idx = (int64_t)(2 * my + (b >> 1)) * (2 * g.mcux) + 2 * mx + (b & 1);
            else idx = (int64_t)(b == 4 ? 4 : 5) * g.nmcu + m;
            const int pred = b < 4 ? py : (b == 4 ? pcb : pcr);
            const int dc = jpeg_code_block(w, h, b < 4 ? 0 : 1, coef + idx * 8, pred);
            if (b < 4) py = dc; else if (b == 4) pcb = dc; else pcr = dc;
        }
    }
    if (w.n > 0) jpeg_put(w, (1u << (8 - w.n)) - 1u, 8 - w.n);
    if (sg != g.nseg - 1) { *w.p++ = 0xff; *w.p++ = (uint8_t)(0xd0 + (sg & 7)); }
    k.seg_len[f * g.nseg + sg] = (int32_t)(w.p - slot);
}

// ---- pass 4: a segment's bytes to their place in the frame's run; `lane` of `lanes` ---------------------------------------------------------------------------
PHC_HD void jpeg_copy_segment(const JpegK& k, int64_t fs, int lane, int lanes) {
    const int64_t f = fs / k.g.nseg;
    const uint8_t* src = k.slots + fs * k.g.slot_bytes;
    uint8_t* dst = k.out + f * k.out_stride + k.seg_off[fs];
    const int len = k.seg_len[fs];
    for (int i = lane; i < len; i += lanes) dst[i] = src[i];
}

}   // namespace phc
