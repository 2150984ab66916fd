/*
 * hvq_scale.h -- what the scale kernel (hvq_scale.hip), the runtime (hvq_scale_pictures) and the tests' fake device share: the weights of
 * the area filter, the exact division by D = nx ny, the choice of the body and the job record of a plane.  Plain C++ that compiles for the
 * host and the device alike.  include/hvqm4_amd.h specifies the values.
 */
#ifndef HVQ_SCALE_H
#define HVQ_SCALE_H

#include <stdint.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_SC_FN __host__ __device__ static inline
#else
#define HVQ_SC_FN static inline
#endif

/* Division of v < 2^27 by m, 1 <= m <= 8192, without a division: with s = ceil(log2 m) and mul = ceil(2^(27 + s) / m) <= 2^28,
 * mul m = 2^(27 + s) + e with 0 <= e < m <= 2^s, so v mul / 2^(27 + s) = v / m + v e / (m 2^(27 + s)), and the second term is below
 * 1 / m because v e < 2^27 2^s: the floor is floor(v / m).  What is divided here is n r and n (r + 1) + m - 1 with n, m <= 8192 and
 * r < m: below 2^26 + 2^13.  shift = 27 + s; tests/test_scale_cpu.py checks the edges of every quotient for every m. */
#define HVQ_SC_DIV_BITS 27u
static inline void hvq_sc_divisor(uint32_t m, uint32_t *mul, uint32_t *shift)
{
    uint32_t s = 0;
    while ((1u << s) < m) ++s;
    *shift = HVQ_SC_DIV_BITS + s;
    *mul = (uint32_t)((((uint64_t)1 << (HVQ_SC_DIV_BITS + s)) + m - 1u) / m);
}
HVQ_SC_FN uint32_t hvq_sc_divm(uint32_t v, uint32_t mul, uint32_t shift) { return (uint32_t)(((uint64_t)v * mul) >> shift); }
/* the first source sample with a share in target sample r when n sources become m targets, and the one past the last; (mul, shift)
 * divide by m */
HVQ_SC_FN uint32_t hvq_sc_first(uint32_t n, uint32_t m, uint32_t r, uint32_t mul, uint32_t shift) { (void)m; return hvq_sc_divm(n * r, mul, shift); }
HVQ_SC_FN uint32_t hvq_sc_end(uint32_t n, uint32_t m, uint32_t r, uint32_t mul, uint32_t shift) { return hvq_sc_divm(n * (r + 1u) + m - 1u, mul, shift); }
/* w(r, y) = max(0, min(m (y + 1), n (r + 1)) - max(m y, n r)) */
HVQ_SC_FN uint32_t hvq_sc_weight(uint32_t n, uint32_t m, uint32_t r, uint32_t y)
{
    const uint32_t hi = m * (y + 1u) < n * (r + 1u) ? m * (y + 1u) : n * (r + 1u);
    const uint32_t lo = m * y > n * r ? m * y : n * r;
    return hi > lo ? hi - lo : 0u;
}

/* Division by D, 16 <= D <= 2^26, of v = S + (D >> 1) < 2^35: magic = ceil(2^64 / D) = (2^64 + e) / D with 0 <= e < D, so
 * v magic / 2^64 = v / D + v e / (D 2^64), and the second term is below v / 2^64 < 2^-29.  The fraction of v / D is at most 1 - 1 / D
 * <= 1 - 2^-26: the sum does not reach the next integer, and the high 64 bits of the product are floor(v / D).  tests/test_scale_cpu.py
 * checks the edges of every quotient against Python's //. */
static inline uint64_t hvq_sc_magic(uint64_t d)
{
    return (uint64_t)((((unsigned __int128)1 << 64) + d - 1u) / d);
}
HVQ_SC_FN uint32_t hvq_sc_div(uint64_t v, uint64_t magic)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__umul64hi(v, magic);
#else
    return (uint32_t)(((unsigned __int128)v * magic) >> 64);
#endif
}

/* the body a plane takes: the direct one when no target sample has more than 2 x 2 taps (identity and enlargement in both directions),
 * the tiled one otherwise.  The values do not depend on it. */
static inline uint32_t hvq_sc_body(uint32_t nx, uint32_t ny, uint32_t mx, uint32_t my)
{
    return nx <= mx && ny <= my ? HVQ_SC_DIRECT : HVQ_SC_TILED;
}

/* the job of a plane; src / dst / pitch as HvqScaleJob says.  force_direct: the direct body whatever the ratio (tests) */
static inline HvqScaleJob hvq_sc_job(uint64_t src, uint32_t pitch, uint32_t nx, uint32_t ny, uint64_t dst, uint32_t mx, uint32_t my, int force_direct)
{
    HvqScaleJob j;
    j.src = src; j.dst = dst; j.pitch = pitch;
    j.nx = nx; j.ny = ny; j.mx = mx; j.my = my;
    j.magic = hvq_sc_magic((uint64_t)nx * ny);
    j.body = force_direct ? HVQ_SC_DIRECT : hvq_sc_body(nx, ny, mx, my);
    const uint32_t tw = j.body == HVQ_SC_TILED ? HVQ_SC_TW : HVQ_SC_DTW, th = j.body == HVQ_SC_TILED ? HVQ_SC_TH : HVQ_SC_DTH;
    j.tiles_x = (mx + tw - 1u) / tw;
    j.tiles = j.tiles_x * ((my + th - 1u) / th);
    if (255ull * nx * ny >= (1ull << 32)) j.body |= HVQ_SC_WIDE;
    /* a tile's row: the sources of min(TW, mx) targets -- at most floor(t nx / mx) + 2 -- behind up to 3 bytes of alignment */
    const uint32_t t = mx < HVQ_SC_TW ? mx : HVQ_SC_TW;
    uint32_t span = (uint32_t)((uint64_t)t * nx / mx) + 2u;
    if (span > nx) span = nx;
    j.row_dwords = (span + 3u + 3u) / 4u;
    j.chunk = HVQ_SC_RAW_DWORDS / j.row_dwords;
    if (j.chunk > HVQ_SC_MAX_CHUNK) j.chunk = HVQ_SC_MAX_CHUNK;
    hvq_sc_divisor(mx, &j.mul_x, &j.shift_x);
    hvq_sc_divisor(my, &j.mul_y, &j.shift_y);
    return j;
}

#endif
