/*
 * hvq_phash.h -- the arithmetic of the perceptual hashes (hvq_picture_hashes, include/hvqm4_amd.h: the specification) that the kernels
 * (hvq_phash.hip) and the CPU fake device of the tests share: the DCT table as committed constants, the weight of a sample in a grid
 * cell, and the record from a picture's cells.  C++ only; everything is constexpr or inline.
 *
 * A picture's cells are uint64 [HVQ_PH_ROWS][HVQ_PH_COLS] (hvq_desc.h): columns 0 .. 31 the 32 x 32 grid S32, columns 32 .. 40 the 32-row x
 * 9-column grid.  By the two identities of the specification 16 S8[r][c] is a 4 x 4 block sum of S32 and 4 D[r][c] a sum of four rows of
 * the 9-column grid, so every comparison of the hashes is made on those sums: 64 S8 > T <=> 64 (16 S8) > sum of all S32, and
 * D[r][c + 1] > D[r][c] <=> 4 D[r][c + 1] > 4 D[r][c].  sum_y = T / 64 = (sum of all S32) / 1024.
 */
#ifndef HVQ_PHASH_H
#define HVQ_PHASH_H

#include <stdint.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_PH_HD __host__ __device__
#else
#define HVQ_PH_HD
#endif

/* C[k][n] = floor(4096 cos((2 n + 1) k pi / 64) + 0.5), rows k = 1 .. 7, n = 0 .. 15 (tests/test_phash_cpu.py: equal to the formula) */
struct HvqPhDct { int32_t c[8][32]; };
constexpr HvqPhDct hvq_ph_dct()
{
    constexpr int32_t half[7][16] = {
        { 4091, 4052, 3973, 3857, 3703, 3513, 3290, 3035, 2751, 2440, 2106, 1751, 1380, 995, 601, 201 },
        { 4076, 3920, 3612, 3166, 2598, 1931, 1189, 401, -401, -1189, -1931, -2598, -3166, -3612, -3920, -4076 },
        { 4052, 3703, 3035, 2106, 995, -201, -1380, -2440, -3290, -3857, -4091, -3973, -3513, -2751, -1751, -601 },
        { 4017, 3406, 2276, 799, -799, -2276, -3406, -4017, -4017, -3406, -2276, -799, 799, 2276, 3406, 4017 },
        { 3973, 3035, 1380, -601, -2440, -3703, -4091, -3513, -2106, -201, 1751, 3290, 4052, 3857, 2751, 995 },
        { 3920, 2598, 401, -1931, -3612, -4076, -3166, -1189, 1189, 3166, 4076, 3612, 1931, -401, -2598, -3920 },
        { 3857, 2106, -601, -3035, -4091, -3290, -995, 1751, 3703, 3973, 2440, -201, -2751, -4052, -3513, -1380 },
    };
    HvqPhDct t{};
    for (int n = 0; n < 32; ++n) t.c[0][n] = 4096;
    for (int k = 1; k < 8; ++k)
        for (int n = 0; n < 16; ++n) {
            t.c[k][n] = half[k - 1][n];
            t.c[k][31 - n] = (k & 1) ? -half[k - 1][n] : half[k - 1][n];       /* C[k][31 - n] = (-1)^k C[k][n] */
        }
    return t;
}

/* w(r, y) = max(0, min(g y + g, n r + n) - max(g y, n r)): the share of sample y in cell r when n samples make g cells (g <= 32, n <= 8192) */
HVQ_PH_HD constexpr uint32_t hvq_ph_weight(uint32_t g, uint32_t n, uint32_t r, uint32_t y)
{
    const int32_t hi = (int32_t)(g * y + g < n * r + n ? g * y + g : n * r + n);
    const int32_t lo = (int32_t)(g * y > n * r ? g * y : n * r);
    return hi > lo ? (uint32_t)(hi - lo) : 0u;
}
/* the samples with a share in cell r: [first, end) */
HVQ_PH_HD constexpr uint32_t hvq_ph_first(uint32_t g, uint32_t n, uint32_t r) { return n * r / g; }
HVQ_PH_HD constexpr uint32_t hvq_ph_end(uint32_t g, uint32_t n, uint32_t r) { return (n * (r + 1u) + g - 1u) / g; }

/* the cell mean in sixteenths */
HVQ_PH_HD constexpr int32_t hvq_ph_mean16(uint64_t cell, uint64_t wh) { return (int32_t)((16u * cell + (wh >> 1)) / wh); }

/* the record from a picture's cells, one value after the other: what hvq_phash_finish_kernel computes with a workgroup.  Host only. */
inline void hvq_phash_record(const uint64_t *cells, uint64_t wh, uint64_t out[4])
{
    constexpr HvqPhDct T = hvq_ph_dct();
    uint64_t total = 0, ah = 0, dh = 0, ph = 0;
    for (uint32_t r = 0; r < 32u; ++r)
        for (uint32_t c = 0; c < 32u; ++c) total += cells[r * HVQ_PH_COLS + c];
    for (uint32_t e = 0; e < 64u; ++e) {
        const uint32_t r = e >> 3, c = e & 7u;
        uint64_t block = 0, d0 = 0, d1 = 0;
        for (uint32_t i = 0; i < 4u; ++i) {
            for (uint32_t j = 0; j < 4u; ++j) block += cells[(4u * r + i) * HVQ_PH_COLS + 4u * c + j];
            d0 += cells[(4u * r + i) * HVQ_PH_COLS + 32u + c];
            d1 += cells[(4u * r + i) * HVQ_PH_COLS + 33u + c];
        }
        ah |= (uint64_t)(64u * block > total) << (63u - e);
        dh |= (uint64_t)(d1 > d0) << (63u - e);
    }
    int64_t g[32][8], f[64];
    for (uint32_t r = 0; r < 32u; ++r)
        for (uint32_t l = 0; l < 8u; ++l) {
            int64_t s = 0;
            for (uint32_t c = 0; c < 32u; ++c) s += (int64_t)T.c[l][c] * hvq_ph_mean16(cells[r * HVQ_PH_COLS + c], wh);
            g[r][l] = s;
        }
    for (uint32_t k = 0; k < 8u; ++k)
        for (uint32_t l = 0; l < 8u; ++l) {
            int64_t s = 0;
            for (uint32_t r = 0; r < 32u; ++r) s += (int64_t)T.c[k][r] * g[r][l];
            f[k * 8u + l] = s;
        }
    int64_t f31 = 0, f32 = 0;                                   /* the values of rank 31 and 32: ties ranked by index */
    for (uint32_t e = 0; e < 64u; ++e) {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < 64u; ++j) rank += f[j] < f[e] || (f[j] == f[e] && j < e);
        if (rank == 31u) f31 = f[e];
        if (rank == 32u) f32 = f[e];
    }
    for (uint32_t e = 0; e < 64u; ++e) ph |= (uint64_t)(2 * f[e] > f31 + f32) << (63u - e);
    out[0] = ah; out[1] = dh; out[2] = ph; out[3] = total / 1024u;
}

#endif
