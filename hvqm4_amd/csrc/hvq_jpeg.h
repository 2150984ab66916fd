/*
 * hvq_jpeg.h -- what the three sides of hvq_encode_jpeg share (include/hvqm4_amd.h: the specification): the kernels (hvq_jpeg.hip), the
 * runtime's header writer (hvq_runtime.cpp) and the CPU body of the fake device (tests/native/fake_jpeg.cpp).  The tables are those of
 * ITU-T T.81: Annex K.1 / K.2 (quantisation), K.3 - K.6 (Huffman), Figure 5 (zigzag); the DCT table is the header text's.  Everything is
 * constexpr: each side uses it where it needs it, nothing is linked.
 */
#ifndef HVQ_JPEG_H
#define HVQ_JPEG_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HVQ_JPEG_FN __host__ __device__ static inline
#else
#define HVQ_JPEG_FN static inline
#endif

#define HVQ_JPEG_HEADER_BYTES 629u      /* SOI .. SOS, the same for every geometry and quality */
#define HVQ_JPEG_HEADER_SLOT  640u      /* a header in an upload: whole 16-byte units */
#define HVQ_JPEG_CODE_BITS    26u       /* the longest code with its value bits: 16 + 10 (AC); DC: 11 + 11 */
#define HVQ_JPEG_DIV_SHIFT    20u       /* hvq_jpeg_div: quotient = n * m >> 20 */
#define HVQ_JPEG_DIV_MAX      1278u     /* ... exact for every n up to this (|F| <= 1151 plus Q >> 1 <= 127) and every Q in 1..255 */

/* natural index (8 * vertical frequency + horizontal frequency) of the k-th coefficient in zigzag order */
static constexpr uint8_t HVQ_JPEG_ZZ[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

/* Annex K.1 and K.2, natural order */
static constexpr uint8_t HVQ_JPEG_QBASE[2][64] = {
    { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
    { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 } };

/* Annex K.3 - K.6: codes per length 1..16 (BITS) and the symbols in code order (HUFFVAL); tables 0 = luminance, 1 = chrominance */
static constexpr uint8_t HVQ_JPEG_DC_BITS[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
static constexpr uint8_t HVQ_JPEG_DC_VALS[2][12] = { { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 }, { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 } };
static constexpr uint8_t HVQ_JPEG_AC_BITS[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 } };
static constexpr uint8_t HVQ_JPEG_AC_VALS[2][162] = {
    { 0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
      0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
      0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
      0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa },
    { 0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
      0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
      0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa } };

/* the first four columns of the DCT table, C[k][n] = floor(s_k cos((2 n + 1) k pi / 16) 8192 + 0.5); C[k][7 - n] = +- C[k][n] */
static constexpr int32_t HVQ_JPEG_C[8][4] = { { 2896, 2896, 2896, 2896 }, { 4017, 3406, 2276, 799 }, { 3784, 1567, -1567, -3784 }, { 3406, -799, -4017, -2276 },
                                              { 2896, -2896, -2896, 2896 }, { 2276, -4017, 799, 3406 }, { 1567, -3784, 3784, -1567 }, { 799, -2276, 3406, -4017 } };

/* the code of every symbol as code << 8 | length, 0 for a symbol the table has not (Annex C: codes of a length count up, a longer
 * length starts at twice the next code).  dc[t][size], ac[t][run << 4 | size] */
struct HvqJpegCodes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr HvqJpegCodes hvq_jpeg_make_codes()
{
    HvqJpegCodes h = {};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < HVQ_JPEG_DC_BITS[t][l - 1]; ++i) h.dc[t][HVQ_JPEG_DC_VALS[t][k++]] = code++ << 8 | (uint32_t)l;
            code <<= 1;
        }
        code = 0; k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < HVQ_JPEG_AC_BITS[t][l - 1]; ++i) h.ac[t][HVQ_JPEG_AC_VALS[t][k++]] = code++ << 8 | (uint32_t)l;
            code <<= 1;
        }
    }
    return h;
}
static constexpr HvqJpegCodes HVQ_JPEG_CODES = hvq_jpeg_make_codes();
static_assert((HVQ_JPEG_CODES.ac[0][0xf0] & 255u) == 11 && (HVQ_JPEG_CODES.ac[1][0xf0] & 255u) == 10 && HVQ_JPEG_CODES.ac[0][0x00] == (0xAu << 8 | 4u) &&
              HVQ_JPEG_CODES.ac[1][0x00] == 2u && HVQ_JPEG_CODES.dc[1][11] == (0x7FEu << 8 | 11u) && HVQ_JPEG_CODES.dc[0][11] == (0x1FEu << 8 | 9u),
              "ZRL, EOB and the longest DC codes of Annex K");

/* IJG scaling of a base table entry */
HVQ_JPEG_FN uint32_t hvq_jpeg_q(uint32_t base, int quality)
{
    const uint32_t s = quality < 50 ? 5000u / (uint32_t)quality : 200u - 2u * (uint32_t)quality;
    const uint32_t q = (base * s + 50u) / 100u;
    return q < 1u ? 1u : q > 255u ? 255u : q;
}

/* Division by a quantiser without dividing: m = hvq_jpeg_recip(Q), then hvq_jpeg_div(n, m) == n / Q for every n <= HVQ_JPEG_DIV_MAX and
 * every Q in 1..255.  m = floor(2^20 / Q) + 1 overshoots 2^20 / Q by e / Q with 0 < e <= Q, so n m / 2^20 = n / Q + n e / (Q 2^20), and
 * the excess stays below 1 / Q -- never reaching the next integer -- while n e < 2^20: 1278 * 255 < 2^19.  n m < 2^31. */
HVQ_JPEG_FN uint32_t hvq_jpeg_recip(uint32_t q) { return (1u << HVQ_JPEG_DIV_SHIFT) / q + 1u; }
HVQ_JPEG_FN uint32_t hvq_jpeg_div(uint32_t n, uint32_t m) { return n * m >> HVQ_JPEG_DIV_SHIFT; }

/* a quantiser as the kernels take it: the reciprocal with Q >> 1 above it */
HVQ_JPEG_FN uint32_t hvq_jpeg_qpack(uint32_t q) { return hvq_jpeg_recip(q) | (q >> 1) << 24; }
HVQ_JPEG_FN int32_t hvq_jpeg_quantise(int32_t f, uint32_t qpack)
{
    const uint32_t a = (uint32_t)(f < 0 ? -f : f);
    const int32_t v = (int32_t)hvq_jpeg_div(a + (qpack >> 24), qpack & 0xFFFFFFu);
    return f < 0 ? -v : v;
}

/* number of bits of |v|: the size category of a coefficient or a DC difference */
HVQ_JPEG_FN uint32_t hvq_jpeg_size(int32_t v)
{
    uint32_t a = (uint32_t)(v < 0 ? -v : v), s = 0;
    while (a) { ++s; a >>= 1; }
    return s;
}

/* MCUs of a row and MCU rows */
HVQ_JPEG_FN uint32_t hvq_jpeg_mw(uint32_t w, uint32_t hs) { return (w + 8u * hs - 1u) / (8u * hs); }
HVQ_JPEG_FN uint32_t hvq_jpeg_mh(uint32_t h, uint32_t vs) { return (h + 8u * vs - 1u) / (8u * vs); }

/* the length no file exceeds: the header, per interval its blocks at HVQ_JPEG_CODE_BITS bits a coefficient rounded up to a byte and
 * every byte stuffed, the RST markers between the intervals, EOI */
static inline uint64_t hvq_jpeg_bound_of(uint32_t w, uint32_t h, uint32_t hs, uint32_t vs)
{
    const uint64_t mw = hvq_jpeg_mw(w, hs), mh = hvq_jpeg_mh(h, vs);
    const uint64_t interval = (mw * (hs * vs + 2u) * 64u * HVQ_JPEG_CODE_BITS + 7u) / 8u;
    return HVQ_JPEG_HEADER_BYTES + 2u + 2u * (mh - 1u) + 2u * mh * interval;
}

/* the HVQ_JPEG_HEADER_BYTES bytes in front of the entropy data (host) */
static inline size_t hvq_jpeg_write_header(uint32_t w, uint32_t h, uint32_t hs, uint32_t vs, int quality, uint8_t *dst)
{
    uint8_t *p = dst;
    static const uint8_t app0[] = { 0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 };
    for (uint8_t b : app0) *p++ = b;
    for (uint32_t t = 0; t < 2; ++t) {
        *p++ = 0xFF; *p++ = 0xDB; *p++ = 0; *p++ = 67; *p++ = (uint8_t)t;
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)hvq_jpeg_q(HVQ_JPEG_QBASE[t][HVQ_JPEG_ZZ[k]], quality);
    }
    const uint8_t sof[] = { 0xFF, 0xC0, 0, 17, 8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3, 1, (uint8_t)(hs << 4 | vs), 0, 2, 0x11, 1, 3, 0x11, 1 };
    for (uint8_t b : sof) *p++ = b;
    for (uint32_t t = 0; t < 2; ++t) {
        *p++ = 0xFF; *p++ = 0xC4; *p++ = 0; *p++ = 19 + 12; *p++ = (uint8_t)t;
        for (int i = 0; i < 16; ++i) *p++ = HVQ_JPEG_DC_BITS[t][i];
        for (int i = 0; i < 12; ++i) *p++ = HVQ_JPEG_DC_VALS[t][i];
        *p++ = 0xFF; *p++ = 0xC4; *p++ = 0; *p++ = 19 + 162; *p++ = (uint8_t)(0x10 | t);
        for (int i = 0; i < 16; ++i) *p++ = HVQ_JPEG_AC_BITS[t][i];
        for (int i = 0; i < 162; ++i) *p++ = HVQ_JPEG_AC_VALS[t][i];
    }
    const uint32_t mw = hvq_jpeg_mw(w, hs);
    const uint8_t tail[] = { 0xFF, 0xDD, 0, 4, (uint8_t)(mw >> 8), (uint8_t)mw, 0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0 };
    for (uint8_t b : tail) *p++ = b;
    return (size_t)(p - dst);
}

#endif
