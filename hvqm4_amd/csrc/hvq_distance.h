/*
 * hvq_distance.h -- what the distance kernels (hvq_distance.hip), the runtime (hvq_distance_pictures, hvq_distance_mask) and the tests'
 * fake device share: the job records, the column walk, the staging and the outward search of the row pass, the exact integer square
 * root and the mask of a dword, written per lane: a kernel calls a phase with its lane and puts a barrier behind it where one is needed,
 * the fake device calls it for every lane in turn.  C++ that compiles for the host and the device alike: integers only.
 * include/hvqm4_amd.h specifies the values.
 *
 * The transform is separable.  With g(x, y) the vertical distance from (x, y) to the nearest background sample of column x (the rows -1
 * and Ny count under border = 1; no such sample: infinite), the value at a foreground sample is the minimum over x' of
 *     (x - x')^2 + g(x', y)^2      EUCLID2
 *     |x - x'| + g(x', y)          CITY
 *     max(|x - x'|, g(x', y))      CHESS
 * because each of the three grows with g for a fixed |x - x'|; under border = 1 the columns -1 and Nx join with g = 0.  The column pass
 * writes g into the map, 0xFFFFFFFF for infinite; the row pass stages the g of whole rows into LDS as uint16 (g <= 8192; HVQ_DT_INF for
 * infinite) and overwrites the rows in place behind a barrier.
 *
 * The search of a sample walks outwards, d = 1, 2, ..., and stops when no x' at distance d or beyond can win: when d^2 (EUCLID2) or d
 * (CITY, CHESS) has reached the best value so far, or when d passes both ends of the row.  So every loop is bounded by Nx, a background
 * sample ends at once, and a foreground sample takes about as many steps as its result is far.
 */
#ifndef HVQ_DISTANCE_H
#define HVQ_DISTANCE_H

#include <stdint.h>

#include "hvq_desc.h"

#define HVQ_DT_EUCLID2 0u                                             /* HVQ_DST_* of include/hvqm4_amd.h */
#define HVQ_DT_CITY    1u
#define HVQ_DT_CHESS   2u
#define HVQ_DT_NONE    0xFFFFFFFFu                                    /* HVQ_DST_NONE */

/* ------------------------------------------------------------------------------------------------ the jobs (host) */
static inline HvqDistanceJob hvq_dt_job(uint64_t src, uint64_t dist, uint32_t nx, uint32_t ny, uint32_t lo, uint32_t hi, uint32_t metric,
                                        uint32_t border)
{
    HvqDistanceJob j;
    j.src = src; j.dist = dist;
    j.nx = nx; j.ny = ny;                                            /* nx is a multiple of 4, at most HVQ_DT_SPAN */
    j.lo = lo; j.hi = hi; j.metric = metric; j.border = border;
    j.colgroups = (nx + HVQ_DT_COLS - 1u) / HVQ_DT_COLS;
    j.rows = HVQ_DT_SPAN / nx < ny ? HVQ_DT_SPAN / nx : ny;
    j.rowgroups = (ny + j.rows - 1u) / j.rows;
    j.pad[0] = j.pad[1] = j.pad[2] = 0u;
    return j;
}

static inline HvqDistMaskJob hvq_dm_job(uint64_t dist, uint64_t dst, uint32_t nx, uint32_t ny, uint32_t body, uint32_t lo, uint32_t hi,
                                        uint32_t invert)
{
    const int fill = body == HVQ_DM_FILL;
    HvqDistMaskJob j;
    j.dist = fill ? 0u : dist; j.dst = dst;
    j.dwords = (nx >> 2) * ny;
    j.tiles = (j.dwords + HVQ_MP_TILE - 1u) / HVQ_MP_TILE;
    j.body = body;
    j.lo = fill ? 0u : lo; j.hi = fill ? 0u : hi; j.invert = fill ? 0u : invert;
    j.pad[0] = j.pad[1] = 0u;
    return j;
}

/* ------------------------------------------------------------------------------------------------ the lanes' code */
#if defined(HVQ_DT_PLAIN) || defined(__HIPCC__)

#if defined(HVQ_DT_PLAIN)
#define HVQ_DT_FN static inline
#define HVQ_DT_UNROLL
#define HVQ_DT_UNROLL4
#else
#define HVQ_DT_FN __device__ static inline __attribute__((always_inline))
#define HVQ_DT_UNROLL _Pragma("unroll")
#define HVQ_DT_UNROLL4 _Pragma("unroll 4")
#endif

/* sixteen bytes of the map: four entries of a row (nx is a multiple of 4 and the map a multiple of 16) */
typedef struct __attribute__((aligned(16))) HvqDtQuad { uint32_t v[4]; } HvqDtQuad;
/* ... and their four staged values */
typedef struct __attribute__((aligned(8))) HvqDtHalf { uint16_t v[4]; } HvqDtHalf;

/* the exact floor square root of any uint32: one binary digit a step, sixteen steps */
HVQ_DT_FN uint32_t hvq_dt_isqrt(uint32_t v)
{
    uint32_t r = 0u;
    HVQ_DT_UNROLL
    for (uint32_t b = 1u << 30; b; b >>= 2) {
        if (v >= r + b) { v -= r + b; r = (r >> 1) + b; }
        else r >>= 1;
    }
    return r;
}

/* ---- launch 1: the columns.  Lane `lane` of column group `group` owns the columns x .. x + 3 and walks them down, then up: g counts the
 * rows since the last background sample (from the border row under border = 1, from nowhere otherwise: HVQ_DT_NONE), the way up takes
 * the smaller of the two.  A wave reads 256 and writes 1024 consecutive bytes a row.  Background is exactly where the way down left 0. */
HVQ_DT_FN void hvq_dt_column(const HvqDistanceJob &J, uint32_t group, uint32_t lane)
{
    const uint32_t x = group * HVQ_DT_COLS + lane * 4u;
    if (x >= J.nx) return;
    const uint32_t step = J.nx >> 2, start = J.border ? 0u : HVQ_DT_NONE;
    const uint32_t *A = (const uint32_t *)(uintptr_t)J.src + (x >> 2);
    HvqDtQuad *D = (HvqDtQuad *)((uint32_t *)(uintptr_t)J.dist + x);
    uint32_t g0 = start, g1 = start, g2 = start, g3 = start;
    HVQ_DT_UNROLL4
    for (uint32_t y = 0; y < J.ny; ++y) {
        const uint32_t v = A[(uint64_t)y * step];
        const uint32_t a0 = v & 255u, a1 = (v >> 8) & 255u, a2 = (v >> 16) & 255u, a3 = v >> 24;
        g0 = a0 >= J.lo && a0 <= J.hi ? g0 + (g0 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        g1 = a1 >= J.lo && a1 <= J.hi ? g1 + (g1 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        g2 = a2 >= J.lo && a2 <= J.hi ? g2 + (g2 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        g3 = a3 >= J.lo && a3 <= J.hi ? g3 + (g3 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        HvqDtQuad q;
        q.v[0] = g0; q.v[1] = g1; q.v[2] = g2; q.v[3] = g3;
        D[(uint64_t)y * step] = q;
    }
    g0 = g1 = g2 = g3 = start;
    HVQ_DT_UNROLL4
    for (uint32_t y = J.ny; y-- > 0u;) {
        HvqDtQuad q = D[(uint64_t)y * step];
        g0 = q.v[0] ? g0 + (g0 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        g1 = q.v[1] ? g1 + (g1 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        g2 = q.v[2] ? g2 + (g2 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        g3 = q.v[3] ? g3 + (g3 != HVQ_DT_NONE ? 1u : 0u) : 0u;
        q.v[0] = g0 < q.v[0] ? g0 : q.v[0]; q.v[1] = g1 < q.v[1] ? g1 : q.v[1];
        q.v[2] = g2 < q.v[2] ? g2 : q.v[2]; q.v[3] = g3 < q.v[3] ? g3 : q.v[3];
        D[(uint64_t)y * step] = q;
    }
}

/* ---- launch 2: the rows.  Row group `group` is the rows group * rows .. of the plane: `hvq_dt_row_samples` consecutive samples of the
 * map, at most HVQ_DT_SPAN, staged into G[HVQ_DT_SPAN] in rounds of HVQ_DT_LANES * 4. */
HVQ_DT_FN uint32_t hvq_dt_row_samples(const HvqDistanceJob &J, uint32_t group)
{
    const uint32_t y0 = group * J.rows, left = J.ny - y0;
    return (left < J.rows ? left : J.rows) * J.nx;
}

/* the lane's four samples of round `round`: from the map into G */
HVQ_DT_FN void hvq_dt_row_stage(const HvqDistanceJob &J, uint32_t group, uint32_t round, uint32_t lane, uint16_t *G)
{
    const uint32_t i = (round * HVQ_DT_LANES + lane) * 4u;
    if (i >= hvq_dt_row_samples(J, group)) return;                    /* the samples of a group are a multiple of 4 */
    const HvqDtQuad q = *(const HvqDtQuad *)((const uint32_t *)(uintptr_t)J.dist + (uint64_t)group * J.rows * J.nx + i);
    HvqDtHalf h;
    HVQ_DT_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) h.v[s] = (uint16_t)(q.v[s] < HVQ_DT_INF ? q.v[s] : HVQ_DT_INF);
    *(HvqDtHalf *)(G + i) = h;
}

template <uint32_t METRIC>
HVQ_DT_FN uint32_t hvq_dt_cost(uint32_t d, uint32_t g)
{
    return METRIC == HVQ_DT_EUCLID2 ? d * d + g * g : METRIC == HVQ_DT_CITY ? d + g : d > g ? d : g;
}

/* the value at sample x of the staged row R[nx] */
template <uint32_t METRIC>
HVQ_DT_FN uint32_t hvq_dt_search(const uint16_t *R, uint32_t nx, uint32_t x, uint32_t border)
{
    const uint32_t g = R[x];
    if (!g) return 0u;                                                /* background */
    uint32_t best = g == HVQ_DT_INF ? HVQ_DT_NONE : hvq_dt_cost<METRIC>(0u, g);
    if (border) {
        const uint32_t e = x + 1u < nx - x ? x + 1u : nx - x, c = hvq_dt_cost<METRIC>(e, 0u);
        best = c < best ? c : best;
    }
    const uint32_t left = x, right = nx - 1u - x, far = left > right ? left : right;
    for (uint32_t d = 1u; d <= far; ++d) {
        if ((METRIC == HVQ_DT_EUCLID2 ? d * d : d) >= best) break;    /* nothing at d or beyond is nearer */
        if (d <= left) {
            const uint32_t a = R[x - d], c = hvq_dt_cost<METRIC>(d, a);
            if (a != HVQ_DT_INF && c < best) best = c;
        }
        if (d <= right) {
            const uint32_t a = R[x + d], c = hvq_dt_cost<METRIC>(d, a);
            if (a != HVQ_DT_INF && c < best) best = c;
        }
    }
    return best;
}

/* sample u (0 .. 3) of lane `lane` in round `round`: its index in the group, consecutive over the lanes; the caller drops what is not
 * below hvq_dt_row_samples */
HVQ_DT_FN uint32_t hvq_dt_row_index(uint32_t round, uint32_t u, uint32_t lane) { return (round * 4u + u) * HVQ_DT_LANES + lane; }

/* the lane's samples of round `round`: searched in G, stored over the map.  Only behind the barrier that ends the staging */
template <uint32_t METRIC>
HVQ_DT_FN void hvq_dt_row_store(const HvqDistanceJob &J, uint32_t group, uint32_t round, uint32_t lane, const uint16_t *G)
{
    const uint32_t n = hvq_dt_row_samples(J, group);
    uint32_t *D = (uint32_t *)(uintptr_t)J.dist + (uint64_t)group * J.rows * J.nx;
    HVQ_DT_UNROLL
    for (uint32_t u = 0; u < 4u; ++u) {
        const uint32_t i = hvq_dt_row_index(round, u, lane);
        if (i >= n) continue;
        const uint32_t r = i / J.nx, x = i - r * J.nx;
        D[i] = hvq_dt_search<METRIC>(G + r * J.nx, J.nx, x, J.border);
    }
}

/* ---- the mask: the four samples of dword d of the Y plane */
HVQ_DT_FN uint32_t hvq_dm_dword(const HvqDistMaskJob &J, uint32_t d)
{
    const HvqDtQuad e = *(const HvqDtQuad *)((const uint32_t *)(uintptr_t)J.dist + 4u * (uint64_t)d);
    uint32_t out = 0u;
    HVQ_DT_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint32_t v = e.v[s];
        uint32_t y;
        if (J.body == HVQ_DM_ROOT) y = v >= 255u * 255u ? 255u : hvq_dt_isqrt(v);
        else y = ((v >= J.lo && v <= J.hi ? 1u : 0u) ^ J.invert) & 1u ? 255u : 0u;
        out |= y << (8u * s);
    }
    return out;
}

#endif
#endif
