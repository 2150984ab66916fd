/*
 * hvq_integral.h -- what the integral kernels (hvq_integral.hip), the runtime (hvq_integral_pictures, hvq_window_pictures, hvq_rect_sums)
 * and the tests' fake device share: the job records, the sums of a dword, the step of the wave prefix, the column walk, the box of a
 * window from the four corners of the tables, the rounded mean, the integer deviation and the threshold, and the sums of a rectangle,
 * written per lane: a kernel calls a phase with its lane and passes the values of the lanes below through the wave's shuffle, the fake
 * device calls it for every lane in turn and passes them through an array.  C++ that compiles for the host and the device alike:
 * integers only, no division.  include/hvqm4_amd.h specifies the values.
 *
 * The tables are inclusive: S(x, y) is the sum over x' <= x, y' <= y, uint32 and so modulo 2^32; Q(x, y) the sum of squares, uint64,
 * which never wraps.  The sum of a box x0 .. x1, y0 .. y1 is S(x1, y1) - S(x0 - 1, y1) - S(x1, y0 - 1) + S(x0 - 1, y0 - 1) in uint32
 * arithmetic, a table read at -1 being 0: exact while the box holds at most HVQ_WN_MAX_AREA = 2^24 samples, because 255 * 2^24 < 2^32.
 *
 * Every loop is bounded: the row pass by the chunks of a row, the column pass by the rows, the mean by eight and the deviation by seven
 * binary digits.
 */
#ifndef HVQ_INTEGRAL_H
#define HVQ_INTEGRAL_H

#include <stdint.h>

#include "hvq_desc.h"

/* ------------------------------------------------------------------------------------------------ the jobs (host) */
static inline HvqIntegralJob hvq_ig_job(uint64_t src, uint64_t sums, uint64_t squares, uint32_t nx, uint32_t ny)
{
    HvqIntegralJob j;
    j.src = src; j.sums = sums; j.squares = squares;
    j.nx = nx; j.ny = ny;                                            /* nx is a multiple of 4 */
    j.rowgroups = (ny + HVQ_IG_WAVES - 1u) / HVQ_IG_WAVES;
    j.colgroups = (nx + HVQ_IG_COLS - 1u) / HVQ_IG_COLS;
    j.chunks = (nx + HVQ_IG_CHUNK - 1u) / HVQ_IG_CHUNK;
    j.pad = 0u;
    return j;
}

/* does a rule of that mode and k read Q? */
static inline int hvq_wn_needs_squares(uint32_t mode, int32_t k) { return mode == HVQ_WN_DEVIATION || (mode == HVQ_WN_THRESHOLD && k != 0); }

static inline HvqWindowJob hvq_wn_job(uint64_t src, uint64_t sums, uint64_t squares, uint64_t dst, uint32_t nx, uint32_t ny, uint32_t cdwords, uint32_t mode,
                                      uint32_t rx, uint32_t ry, int32_t k, int32_t c, uint32_t invert)
{
    HvqWindowJob j;
    j.src = src; j.sums = sums; j.squares = hvq_wn_needs_squares(mode, k) ? squares : 0u; j.dst = dst;
    j.nx = nx; j.ny = ny;
    j.tx = (nx + HVQ_WN_TX - 1u) / HVQ_WN_TX;
    j.ytiles = j.tx * ((ny + HVQ_WN_TY - 1u) / HVQ_WN_TY);
    j.cdwords = cdwords;
    j.tiles = j.ytiles + (cdwords + HVQ_WN_LANES * HVQ_WN_PER - 1u) / (HVQ_WN_LANES * HVQ_WN_PER);
    j.mode = mode; j.rx = rx; j.ry = ry; j.k = k; j.c = c; j.invert = invert;
    return j;
}

/* ------------------------------------------------------------------------------------------------ the lanes' code */
#if defined(HVQ_IG_PLAIN) || defined(__HIPCC__)

#if defined(HVQ_IG_PLAIN)
#define HVQ_IG_FN static inline
#define HVQ_IG_UNROLL
#define HVQ_IG_UNROLL4
#else
#define HVQ_IG_FN __device__ static inline __attribute__((always_inline))
#define HVQ_IG_UNROLL _Pragma("unroll")
#define HVQ_IG_UNROLL4 _Pragma("unroll 4")
#endif

/* sixteen bytes of a table: four entries of S, two of Q (nx is a multiple of 4 and the tables multiples of 16) */
typedef struct __attribute__((aligned(16))) HvqIgQuad { uint32_t v[4]; } HvqIgQuad;
typedef struct __attribute__((aligned(16))) HvqIgPair { uint64_t v[2]; } HvqIgPair;

/* ---- launch 1: the rows.  Lane `lane` of the wave that owns row y takes, in chunk c, the dword of the samples x .. x + 3, x = c *
 * HVQ_IG_CHUNK + lane * 4: 0 past the row's end, which adds nothing */
HVQ_IG_FN uint32_t hvq_ig_row_load(const HvqIntegralJob &J, uint32_t y, uint32_t chunk, uint32_t lane)
{
    const uint32_t x = chunk * HVQ_IG_CHUNK + lane * 4u;
    return x < J.nx ? ((const uint32_t *)(uintptr_t)J.src)[((uint64_t)y * J.nx + x) >> 2] : 0u;
}

/* the sum of the four samples of a dword, and of their squares */
HVQ_IG_FN uint32_t hvq_ig_sum4(uint32_t v) { return (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24); }
HVQ_IG_FN uint32_t hvq_ig_sq4(uint32_t v)
{
    const uint32_t a0 = v & 255u, a1 = (v >> 8) & 255u, a2 = (v >> 16) & 255u, a3 = v >> 24;
    return a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
}

/* one step of the wave's inclusive prefix (delta = 1, 2, 4 .. HVQ_IG_WAVE / 2): `below` is the value lane - delta held before the step */
HVQ_IG_FN uint32_t hvq_ig_scan_step(uint32_t v, uint32_t below, uint32_t lane, uint32_t delta) { return lane >= delta ? v + below : v; }
HVQ_IG_FN uint64_t hvq_ig_scan_step64(uint64_t v, uint64_t below, uint32_t lane, uint32_t delta) { return lane >= delta ? v + below : v; }

/* the lane's four entries of row y: `before` and `qbefore` are the sums of everything left of x in the row (the carry of the chunks
 * before plus the totals of the lanes below) */
HVQ_IG_FN void hvq_ig_row_store(const HvqIntegralJob &J, uint32_t y, uint32_t chunk, uint32_t lane, uint32_t v, uint32_t before, uint64_t qbefore)
{
    const uint32_t x = chunk * HVQ_IG_CHUNK + lane * 4u;
    if (x >= J.nx) return;
    const uint64_t at = (uint64_t)y * J.nx + x;
    const uint32_t a0 = v & 255u, a1 = (v >> 8) & 255u, a2 = (v >> 16) & 255u, a3 = v >> 24;
    HvqIgQuad s;
    s.v[0] = before + a0; s.v[1] = s.v[0] + a1; s.v[2] = s.v[1] + a2; s.v[3] = s.v[2] + a3;
    *(HvqIgQuad *)((uint32_t *)(uintptr_t)J.sums + at) = s;
    if (!J.squares) return;                                           /* uniform */
    HvqIgPair *Q = (HvqIgPair *)((uint64_t *)(uintptr_t)J.squares + at);
    HvqIgPair lo, hi;
    lo.v[0] = qbefore + a0 * a0; lo.v[1] = lo.v[0] + a1 * a1;
    hi.v[0] = lo.v[1] + a2 * a2; hi.v[1] = hi.v[0] + a3 * a3;
    Q[0] = lo; Q[1] = hi;
}

/* ---- launch 2: the columns.  Lane `lane` of column group `group` owns the columns x .. x + 3 and adds the rows' prefixes downwards, in
 * place: a wave reads and writes 1024 consecutive bytes of S a row, 2048 of Q. */
HVQ_IG_FN void hvq_ig_column(const HvqIntegralJob &J, uint32_t group, uint32_t lane)
{
    const uint32_t x = group * HVQ_IG_COLS + lane * 4u;
    if (x >= J.nx) return;
    const uint32_t step = J.nx >> 2;
    HvqIgQuad *S = (HvqIgQuad *)((uint32_t *)(uintptr_t)J.sums + x);
    uint32_t s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u;
    HVQ_IG_UNROLL4
    for (uint32_t y = 0; y < J.ny; ++y) {
        HvqIgQuad q = S[(uint64_t)y * step];
        s0 += q.v[0]; s1 += q.v[1]; s2 += q.v[2]; s3 += q.v[3];
        q.v[0] = s0; q.v[1] = s1; q.v[2] = s2; q.v[3] = s3;
        S[(uint64_t)y * step] = q;
    }
    if (!J.squares) return;                                           /* uniform */
    HvqIgPair *Q = (HvqIgPair *)((uint64_t *)(uintptr_t)J.squares + x);
    uint64_t q0 = 0u, q1 = 0u, q2 = 0u, q3 = 0u;
    HVQ_IG_UNROLL4
    for (uint32_t y = 0; y < J.ny; ++y) {
        HvqIgPair lo = Q[(uint64_t)y * step * 2u], hi = Q[(uint64_t)y * step * 2u + 1u];
        q0 += lo.v[0]; q1 += lo.v[1]; q2 += hi.v[0]; q3 += hi.v[1];
        lo.v[0] = q0; lo.v[1] = q1; hi.v[0] = q2; hi.v[1] = q3;
        Q[(uint64_t)y * step * 2u] = lo; Q[(uint64_t)y * step * 2u + 1u] = hi;
    }
}

/* ---- the window.  The box of sample (x, y) under the radii (rx, ry), cut to the plane: its samples, their sum and, where Qt is not
 * null, their sum of squares, from the four corners; a corner left of column 0 or above row 0 reads as 0 */
HVQ_IG_FN void hvq_wn_box(const uint32_t *St, const uint64_t *Qt, uint32_t nx, uint32_t ny, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t *S, uint64_t *Q)
{
    (void)ny;
    const uint64_t lower = (uint64_t)y1 * nx, upper = (uint64_t)(y0 ? y0 - 1u : 0u) * nx;
    const uint32_t xl = x0 ? x0 - 1u : 0u;
    const uint32_t d = St[lower + x1], c = x0 ? St[lower + xl] : 0u, b = y0 ? St[upper + x1] : 0u, a = x0 && y0 ? St[upper + xl] : 0u;
    *S = d - c - b + a;                                               /* modulo 2^32: exact for a box of at most 2^24 samples */
    if (!Qt) { *Q = 0u; return; }
    const uint64_t qd = Qt[lower + x1], qc = x0 ? Qt[lower + xl] : 0u, qb = y0 ? Qt[upper + x1] : 0u, qa = x0 && y0 ? Qt[upper + xl] : 0u;
    *Q = qd - qc - qb + qa;
}

/* (2 S + n) / (2 n) rounded down, the mean rounded half up, in 0 .. 255: the largest m with m * 2 n <= 2 S + n, a binary digit a step */
HVQ_IG_FN uint32_t hvq_wn_mean(uint32_t S, uint32_t n)
{
    const uint64_t num = 2u * (uint64_t)S + n, den = 2u * (uint64_t)n;
    uint32_t m = 0u;
    HVQ_IG_UNROLL
    for (uint32_t b = 128u; b; b >>= 1)
        if ((uint64_t)(m | b) * den <= num) m |= b;
    return m;
}

/* the largest d with (d n)^2 <= n Q - S^2, the floor of the population standard deviation, in 0 .. 127.  n <= 2^24: n Q and S^2 are
 * below 255^2 * 2^48 < 2^64, and (127 n)^2 < 2^62 */
HVQ_IG_FN uint32_t hvq_wn_deviation(uint32_t S, uint64_t Q, uint32_t n)
{
    const uint64_t var = (uint64_t)n * Q - (uint64_t)S * S;
    uint32_t d = 0u;
    HVQ_IG_UNROLL
    for (uint32_t b = 64u; b; b >>= 1) {
        const uint64_t t = (uint64_t)(d | b) * n;
        if (t * t <= var) d |= b;
    }
    return d;
}

/* the value of sample (x, y) of Y, `a` its own sample (THRESHOLD) */
HVQ_IG_FN uint32_t hvq_wn_value(const HvqWindowJob &J, uint32_t x, uint32_t y, uint32_t a)
{
    const uint32_t x0 = x > J.rx ? x - J.rx : 0u, y0 = y > J.ry ? y - J.ry : 0u;
    const uint32_t x1 = J.nx - 1u - x > J.rx ? x + J.rx : J.nx - 1u, y1 = J.ny - 1u - y > J.ry ? y + J.ry : J.ny - 1u;
    const uint32_t n = (x1 - x0 + 1u) * (y1 - y0 + 1u);
    uint32_t S;
    uint64_t Q;
    hvq_wn_box((const uint32_t *)(uintptr_t)J.sums, (const uint64_t *)(uintptr_t)J.squares, J.nx, J.ny, x0, y0, x1, y1, &S, &Q);
    if (J.mode == HVQ_WN_MEAN) return hvq_wn_mean(S, n);
    if (J.mode == HVQ_WN_DEVIATION) return hvq_wn_deviation(S, Q, n);
    const int64_t d = J.k ? (int64_t)hvq_wn_deviation(S, Q, n) : 0;
    const int64_t lhs = 256 * (int64_t)n * (int64_t)a, rhs = 256 * (int64_t)S + (int64_t)J.k * d * (int64_t)n - 256 * (int64_t)J.c * (int64_t)n;
    return ((lhs > rhs ? 1u : 0u) ^ J.invert) & 1u ? 255u : 0u;
}

/* where lane `lane` of Y tile t stands: its four samples are (x .. x + 3, y); the caller drops what is outside the plane */
HVQ_IG_FN void hvq_wn_place(const HvqWindowJob &J, uint32_t t, uint32_t lane, uint32_t *x, uint32_t *y)
{
    const uint32_t ty = t / J.tx, tx = t - ty * J.tx;
    *x = tx * HVQ_WN_TX + (lane & (HVQ_WN_TX / 4u - 1u)) * 4u;
    *y = ty * HVQ_WN_TY + lane / (HVQ_WN_TX / 4u);
}

/* the dword of the four samples (x .. x + 3, y) of Y */
HVQ_IG_FN uint32_t hvq_wn_dword(const HvqWindowJob &J, uint32_t x, uint32_t y)
{
    const uint32_t v = J.mode == HVQ_WN_THRESHOLD ? ((const uint32_t *)(uintptr_t)J.src)[((uint64_t)y * J.nx + x) >> 2] : 0u;
    uint32_t out = 0u;
    HVQ_IG_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) out |= hvq_wn_value(J, x + s, y, (v >> (8u * s)) & 255u) << (8u * s);
    return out;
}

/* chroma dword u (0 .. HVQ_WN_PER - 1) of lane `lane` in chroma tile t (counted from the first one): its index in U | V; the caller drops
 * what is not below J.cdwords */
HVQ_IG_FN uint32_t hvq_wn_chroma(uint32_t t, uint32_t lane, uint32_t u) { return (t * HVQ_WN_PER + u) * HVQ_WN_LANES + lane; }

/* ---- the rectangles: rectangle r -> out[r] = (count, S, Q); (0, 0, 0) for a picture that is none, corners out of order or outside the
 * plane, or more than HVQ_WN_MAX_AREA samples */
HVQ_IG_FN void hvq_rc_rect(const HvqRectHead &H, const HvqRectTables *T, uint32_t r)
{
    const int32_t *R = (const int32_t *)(uintptr_t)H.rects + 5u * (uint64_t)r;
    uint64_t *O = (uint64_t *)(uintptr_t)H.out + 3u * (uint64_t)r;
    const int32_t i = R[0], x0 = R[1], y0 = R[2], x1 = R[3], y1 = R[4];
    uint64_t count = 0u, Q = 0u;
    uint32_t S = 0u;
    if (i >= 0 && (uint32_t)i < H.npics) {
        const uint32_t *D = (const uint32_t *)(uintptr_t)H.dims + 2u * (uint32_t)i;
        const uint32_t nx = D[0], ny = D[1];
        if (x0 >= 0 && y0 >= 0 && x0 <= x1 && y0 <= y1 && (uint32_t)x1 < nx && (uint32_t)y1 < ny) {
            const uint64_t area = (uint64_t)(uint32_t)(x1 - x0 + 1) * (uint32_t)(y1 - y0 + 1);
            if (area <= HVQ_WN_MAX_AREA) {
                count = area;
                hvq_wn_box((const uint32_t *)(uintptr_t)T[i].sums, (const uint64_t *)(uintptr_t)T[i].squares, nx, ny, (uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1,
                           &S, &Q);
            }
        }
    }
    O[0] = count; O[1] = S; O[2] = Q;
}

#endif
#endif
