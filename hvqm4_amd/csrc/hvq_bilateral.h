/*
 * hvq_bilateral.h -- what the bilateral kernel (hvq_bilateral.hip), the runtime (hvq_bilateral_pictures) and the tests' fake device
 * share: the choice of a plane's body and its job record, the index arithmetic of a tile (which source row and dword a staged dword is,
 * the edge sample in the halo), the tap step of a lane's four targets, the walk of a lane over its window and the exact division,
 * written per lane over the tile's LDS arrays: the kernel calls them with its lane, the fake device for every lane in turn.  Plain C++
 * that compiles for the host and the device alike.  include/hvqm4_amd.h specifies the values.
 *
 * The staged tile.  rows = HVQ_BL_TH + 2 ry staged rows, staged row rr = source row r0 + rr - ry clamped into the plane; each
 * HVQ_BL_ROW_DWORDS aligned dwords, the source bytes c0 - 8 .. c0 + 71.  A dword that lies outside the row holds the row's edge sample
 * four times: rows AND columns are clamped when staging (the rank unit's scheme), so that the tap loop clamps nothing and every window
 * of a target, as the header counts it, lies in the staged bytes as it is.  A second tile, staged the same way, holds the guide plane
 * when the picture has one.
 *
 * 32 bits.  A weight is spatial x range <= 255 * 255 and a sample <= 255: both products are 24 x 24-bit multiply-adds, and with 225 taps
 * num + den / 2 <= 225 * 65025 * 255 + 7315312 < 2^32 (the header's bound).
 */
#ifndef HVQ_BILATERAL_H
#define HVQ_BILATERAL_H

#include <stdint.h>
#include <string.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_BL_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define HVQ_BL_FN static inline
#endif

#define HVQ_BL_MAX_SETS 64u           /* HVQ_BIL_MAX_SETS */

/* ------------------------------------------------------------------------------------------------ the job of a plane (host) */
/* the body of a plane: the copy body for radius 0 in both axes -- the centre tap alone, whose weight is at least 1: (w a + w / 2) / w
 * is a -- unless `general` switches it off (hvq_bilateral_force_general) */
static inline HvqBilateralJob hvq_bl_job(uint64_t src, uint64_t dst, uint64_t guide, uint32_t nx, uint32_t ny, uint32_t ps, uint32_t rx, uint32_t ry, int general)
{
    HvqBilateralJob j;
    memset(&j, 0, sizeof j);
    j.src = src; j.dst = dst; j.guide = guide; j.nx = nx; j.ny = ny; j.ps = ps; j.rx = rx; j.ry = ry;
    j.body = !rx && !ry && !general ? HVQ_BL_COPY : HVQ_BL_GENERAL;
    const uint32_t tw = j.body == HVQ_BL_COPY ? HVQ_BL_CTW : HVQ_BL_TW, th = j.body == HVQ_BL_COPY ? HVQ_BL_CTH : HVQ_BL_TH;
    j.tiles_x = (nx + tw - 1u) / tw;
    j.tiles = j.tiles_x * ((ny + th - 1u) / th);
    return j;
}

/* ------------------------------------------------------------------------------------------------ staging */
HVQ_BL_FN uint32_t hvq_bl_stage_row(uint32_t r0, uint32_t rr, uint32_t ry, uint32_t ny)
{
    const int32_t y = (int32_t)(r0 + rr) - (int32_t)ry;
    return y < 0 ? 0u : y >= (int32_t)ny ? ny - 1u : (uint32_t)y;
}
/* dword k of a staged row is the row's dword c0 / 4 - 2 + k; one outside the row is loaded from the nearest inside ... */
HVQ_BL_FN uint32_t hvq_bl_stage_dword(uint32_t c0, uint32_t k, uint32_t nx)
{
    const int32_t d = (int32_t)(c0 >> 2) - (int32_t)(HVQ_BL_HALO >> 2) + (int32_t)k, last = (int32_t)(nx >> 2) - 1;
    return d < 0 ? 0u : d > last ? (uint32_t)last : (uint32_t)d;
}
/* ... and becomes the edge sample four times: the first byte of the row left of it, the last byte right of it (nx is a multiple of 4: a
 * dword lies inside the row or outside) */
HVQ_BL_FN uint32_t hvq_bl_stage_value(uint32_t v, uint32_t c0, uint32_t k, uint32_t nx)
{
    const int32_t d = (int32_t)(c0 >> 2) - (int32_t)(HVQ_BL_HALO >> 2) + (int32_t)k, last = (int32_t)(nx >> 2) - 1;
    return d < 0 ? (v & 0xffu) * 0x01010101u : d > last ? (v >> 24) * 0x01010101u : v;
}

/* bytes sh .. sh + 3 of the eight bytes lo, hi (sh 0 .. 3): v_alignbyte_b32 */
HVQ_BL_FN uint32_t hvq_bl_align(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (sh & 3u)));
#endif
}
/* the four bytes from byte `at` of an array of aligned dwords: the dword it starts in and the one behind */
HVQ_BL_FN uint32_t hvq_bl_read(const uint32_t *row, uint32_t at) { return hvq_bl_align(row[(at >> 2) + 1u], row[at >> 2], at & 3u); }

/* ------------------------------------------------------------------------------------------------ the taps */
/* row aj of a plane's spatial table, its eight factors in one qword (the table is workgroup-uniform: scalar loads on the device) */
HVQ_BL_FN uint64_t hvq_bl_spatial_row(const uint8_t *spatial, uint32_t aj)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const uint64_t *)spatial)[aj];
#else
    uint64_t v;
    memcpy(&v, spatial + 8u * aj, 8);
    return v;
#endif
}

/* |byte k of g - byte k of c| of two dwords that hold nothing but their byte k: v_sad_u8 sums the four byte differences, three of them 0 */
HVQ_BL_FN uint32_t hvq_bl_absdiff(uint32_t g, uint32_t c, uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)k;
    return __builtin_amdgcn_sad_u8(g, c, 0u);
#else
    const uint32_t a = g >> (8u * k), b = c >> (8u * k);
    return a > b ? a - b : b - a;
#endif
}
/* a product of two factors below 2^24 whose result fits 32 bits: v_mul_u32_u24, and with the sum behind it v_mad_u32_u24 */
HVQ_BL_FN uint32_t hvq_bl_mul24(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}

/* one tap on a lane's four targets: av, gv the neighbour dwords of the source and of the guide, gc[k] the targets' own guide dword with
 * every byte but k cleared, s the tap's spatial factor (not 0), range the plane's 256 range bytes */
HVQ_BL_FN void hvq_bl_tap(uint32_t av, uint32_t gv, const uint32_t gc[4], uint32_t s, const uint8_t *range, uint32_t num[4], uint32_t den[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t d = hvq_bl_absdiff(gv & (0xffu << (8u * k)), gc[k], k);
        const uint32_t w = hvq_bl_mul24(s, (uint32_t)range[d]);      /* <= 65025 */
        den[k] += w;
        num[k] += hvq_bl_mul24(w, (av >> (8u * k)) & 0xffu);
    }
}

/* out = (num + den / 2) / den: floor of the quotient, one rounding, half up; den >= 1 (the centre tap), num + den / 2 < 2^32 */
HVQ_BL_FN uint32_t hvq_bl_finish(uint32_t num, uint32_t den) { return (num + (den >> 1)) / den; }

/* The lane's dword of the tile -- dword lane & 15 of target row lane >> 4 -- from the staged tile A, the staged guide tile G (A itself
 * where the picture guides itself: `guided` 0 then leaves the second read out), the plane's spatial table and its range bytes.  The taps
 * are a double loop whose spatial factor is the same for the whole workgroup; a tap whose factor is 0 is skipped. */
HVQ_BL_FN uint32_t hvq_bl_lane(uint32_t lane, uint32_t rx, uint32_t ry, int guided, const uint8_t *spatial, const uint32_t *A, const uint32_t *G, const uint8_t *range)
{
    const uint32_t lr = lane >> 4, at0 = HVQ_BL_HALO + 4u * (lane & 15u);
    const uint32_t gcv = (guided ? G : A)[(lr + ry) * HVQ_BL_ROW_DWORDS + (at0 >> 2)];
    const uint32_t gc[4] = { gcv & 0xffu, gcv & 0xff00u, gcv & 0xff0000u, gcv & 0xff000000u };
    uint32_t num[4] = { 0u, 0u, 0u, 0u }, den[4] = { 0u, 0u, 0u, 0u };
    for (int32_t j = -(int32_t)ry; j <= (int32_t)ry; ++j) {
        const uint64_t srow = hvq_bl_spatial_row(spatial, (uint32_t)(j < 0 ? -j : j));
        const uint32_t row = (uint32_t)((int32_t)(lr + ry) + j) * HVQ_BL_ROW_DWORDS;
        for (int32_t i = -(int32_t)rx; i <= (int32_t)rx; ++i) {
            const uint32_t s = (uint32_t)(srow >> (8u * (uint32_t)(i < 0 ? -i : i))) & 0xffu;
            if (!s) continue;                                          /* uniform */
            const uint32_t at = (uint32_t)((int32_t)at0 + i);
            const uint32_t av = hvq_bl_read(A + row, at);
            hvq_bl_tap(av, guided ? hvq_bl_read(G + row, at) : av, gc, s, range, num, den);
        }
    }
    return hvq_bl_finish(num[0], den[0]) | hvq_bl_finish(num[1], den[1]) << 8 | hvq_bl_finish(num[2], den[2]) << 16 | hvq_bl_finish(num[3], den[3]) << 24;
}

#endif
