/*
 * hvq_map.h -- what the map and table kernels (hvq_map.hip), the runtime (hvq_map_pictures, hvq_histogram_tables) and the tests' fake
 * device share: the job record of a plane, the index map of a tile, the lookup of the four samples of a dword, and the phases of the
 * table kernel, written per lane over the workgroup's LDS record: the kernel calls a phase with its lane and puts a barrier behind it,
 * the fake device calls it for every lane in turn.  Plain C++ that compiles for the host and the device alike: integers only, no
 * floating point, no 128-bit type.  include/hvqm4_amd.h specifies the values.
 *
 * The map tile.  A point operation does not look at rows: a plane is its nx ny / 4 dwords, and a tile is HVQ_MP_TILE = 2048 consecutive
 * ones (8 KiB).  Lane l of the workgroup takes the dwords l, l + 256, ... l + 7 * 256 of the tile: a wave reads and writes 256 adjacent
 * bytes an instruction.  The workgroup stages its plane's 256 table bytes once: 32 samples are looked up for every byte staged.
 *
 * The staged table.  HVQ_MP_WIDE 0: the 256 bytes as they are (64 dwords), a sample a reads byte a.  HVQ_MP_WIDE 1: one dword an entry
 * (1 KiB), a sample a reads dword a: entry a lies in bank a mod 32 instead of (a / 4) mod 32.  DESIGN.md 4.5 says which one is built
 * and why.
 */
#ifndef HVQ_MAP_H
#define HVQ_MAP_H

#include <stdint.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_MP_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define HVQ_MP_FN static inline
#endif

#ifndef HVQ_MP_WIDE
#define HVQ_MP_WIDE 0
#endif
#if HVQ_MP_WIDE
typedef uint32_t HvqMpEntry;
#else
typedef uint8_t HvqMpEntry;
#endif

/* the table kinds of include/hvqm4_amd.h (HVQ_TBL_*) */
#define HVQ_TB_IDENTITY 0u
#define HVQ_TB_FLAT     1u
#define HVQ_TB_EQUALIZE 2u
#define HVQ_TB_STRETCH  3u
#define HVQ_TB_OTSU     4u

/* ------------------------------------------------------------------------------------------------ the job of a plane (host) */
static inline HvqMapJob hvq_mp_job(uint64_t src, uint64_t dst, uint64_t table, uint32_t nx, uint32_t ny, int lookup)
{
    HvqMapJob j;
    j.src = src; j.dst = dst; j.table = lookup ? table : 0u;
    j.dwords = (nx >> 2) * ny;                                       /* nx is a multiple of 4 */
    j.tiles = (j.dwords + HVQ_MP_TILE - 1u) / HVQ_MP_TILE;
    j.body = lookup ? HVQ_MP_LOOKUP : HVQ_MP_COPY;
    j.pad[0] = j.pad[1] = j.pad[2] = 0u;
    return j;
}

/* ------------------------------------------------------------------------------------------------ the tile */
/* dword u (0 .. HVQ_MP_PER - 1) of lane `lane` in tile t: its index in the plane; the caller drops what is not below J.dwords */
HVQ_MP_FN uint32_t hvq_mp_dword(uint32_t t, uint32_t lane, uint32_t u) { return t * HVQ_MP_TILE + u * HVQ_MP_LANES + lane; }

/* the four samples of a dword through the staged table */
HVQ_MP_FN uint32_t hvq_mp_lookup4(const HvqMpEntry *T, uint32_t v)
{
    return (uint32_t)T[v & 255u] | (uint32_t)T[(v >> 8) & 255u] << 8 | (uint32_t)T[(v >> 16) & 255u] << 16 | (uint32_t)T[v >> 24] << 24;
}

/* ------------------------------------------------------------------------------------------------ the table kernel
 * Lane v holds bin v.  C(v) = sum of h[0 .. v] and S(v) = sum of u h[u] over the same come from an inclusive scan of eight doubling
 * steps between two arrays (a barrier behind each).  What a table needs besides them is a value that exactly ONE lane knows -- the count
 * of the smallest occurring value, the sample of a rank: the lane where C first reaches the rank -- so that lane writes it into sel[]
 * and nobody reduces; only Otsu's arg-max is a reduction, a tree of eight steps over candidates whose comparison is a total order. */
typedef struct HvqTbLds {
    uint32_t cnt[2][256];          /* the scan of the counts: the result stands in cnt[0] */
    uint64_t sum[2][256];          /* the scan of v h[v] */
    uint64_t d2h[256], d2l[256];   /* Otsu candidate t = lane: d^2, 128 bits */
    uint64_t m[256];               /*                          n0 n1 */
    uint32_t t[256], valid[256];
    uint32_t sel[4];               /* C_min; lo; hi */
} HvqTbLds;

HVQ_MP_FN void hvq_tb_load(HvqTbLds *L, uint32_t lane, uint32_t h)
{
    L->cnt[0][lane] = h;
    L->sum[0][lane] = (uint64_t)lane * h;
    if (lane < 4u) L->sel[lane] = 0u;
}
/* step k = 0 .. 7 of the scan: from array k & 1 into the other; after the eighth the result stands in array 0 */
HVQ_MP_FN void hvq_tb_scan(HvqTbLds *L, uint32_t lane, uint32_t k)
{
    const uint32_t f = k & 1u, s = 1u << k;
    L->cnt[f ^ 1u][lane] = L->cnt[f][lane] + (lane >= s ? L->cnt[f][lane - s] : 0u);
    L->sum[f ^ 1u][lane] = L->sum[f][lane] + (lane >= s ? L->sum[f][lane - s] : 0u);
}

/* a 64 x 64 -> 128 bit product from 32-bit pieces */
HVQ_MP_FN void hvq_tb_mul64(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo)
{
    const uint64_t al = a & 0xffffffffu, ah = a >> 32, bl = b & 0xffffffffu, bh = b >> 32;
    const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
    const uint64_t mid = (ll >> 32) + (lh & 0xffffffffu) + (hl & 0xffffffffu);
    *lo = (ll & 0xffffffffu) | mid << 32;
    *hi = hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}
/* (h, l) x m -> three limbs, r[2] the highest: d^2 < 2^116 and m < 2^52 keep it below 2^168 */
HVQ_MP_FN void hvq_tb_mul192(uint64_t h, uint64_t l, uint64_t m, uint64_t r[3])
{
    uint64_t p0h, p0l, p1h, p1l;
    hvq_tb_mul64(l, m, &p0h, &p0l);
    hvq_tb_mul64(h, m, &p1h, &p1l);
    r[0] = p0l;
    r[1] = p0h + p1l;
    r[2] = p1h + (r[1] < p0h ? 1u : 0u);
}
/* the rank of `pm` per mille of N samples: max(1, ceil(pm N / 1000)) */
HVQ_MP_FN uint32_t hvq_tb_rank(uint32_t pm, uint32_t N)
{
    const uint64_t k = ((uint64_t)pm * N + 999u) / 1000u;
    return k ? (uint32_t)k : 1u;
}

/* what one lane knows: C_min, the samples at the clip ranks, and the lane's Otsu candidate */
HVQ_MP_FN void hvq_tb_select(HvqTbLds *L, uint32_t lane, uint32_t kind, uint32_t a, uint32_t b)
{
    const uint32_t C = L->cnt[0][lane], prev = lane ? L->cnt[0][lane - 1u] : 0u, N = L->cnt[0][255];
    if (kind == HVQ_TB_EQUALIZE) {
        if (C && !prev) L->sel[0] = C;
    } else if (kind == HVQ_TB_STRETCH) {
        const uint32_t klo = hvq_tb_rank(a, N), khi = hvq_tb_rank(1000u - b, N);
        if (C >= klo && prev < klo) L->sel[1] = lane;
        if (C >= khi && prev < khi) L->sel[2] = lane;
    } else if (kind == HVQ_TB_OTSU) {
        const uint64_t n0 = C, n1 = N - C, s0 = L->sum[0][lane], s1 = L->sum[0][255] - s0;
        uint64_t d = s0 * n1 - s1 * n0;
        if (d >> 63) d = 0u - d;                                     /* |d| */
        hvq_tb_mul64(d, d, &L->d2h[lane], &L->d2l[lane]);
        L->m[lane] = n0 * n1;
        L->t[lane] = lane;
        L->valid[lane] = lane < 255u && C && N != C ? 1u : 0u;
    }
}
/* is candidate j better than candidate i?  A total order: a valid one before an invalid one, then the larger d^2 / m -- compared as
 * d_j^2 m_i against d_i^2 m_j --, then the smaller t */
HVQ_MP_FN int hvq_tb_better(const HvqTbLds *L, uint32_t j, uint32_t i)
{
    if (L->valid[j] != L->valid[i]) return L->valid[j] > L->valid[i];
    if (L->valid[j]) {
        uint64_t x[3], y[3];
        hvq_tb_mul192(L->d2h[j], L->d2l[j], L->m[i], x);
        hvq_tb_mul192(L->d2h[i], L->d2l[i], L->m[j], y);
        if (x[2] != y[2]) return x[2] > y[2];
        if (x[1] != y[1]) return x[1] > y[1];
        if (x[0] != y[0]) return x[0] > y[0];
    }
    return L->t[j] < L->t[i];
}
/* a step of the tree, s = 128, 64 .. 1: the lanes below s keep the better of their candidate and the one s further on (which no lane
 * writes in this step) */
HVQ_MP_FN void hvq_tb_reduce(HvqTbLds *L, uint32_t lane, uint32_t s)
{
    if (lane >= s || !hvq_tb_better(L, lane + s, lane)) return;
    L->d2h[lane] = L->d2h[lane + s]; L->d2l[lane] = L->d2l[lane + s]; L->m[lane] = L->m[lane + s];
    L->t[lane] = L->t[lane + s]; L->valid[lane] = L->valid[lane + s];
}
/* entry `lane` of the table */
HVQ_MP_FN uint8_t hvq_tb_value(const HvqTbLds *L, uint32_t lane, uint32_t kind, uint32_t a)
{
    if (kind == HVQ_TB_FLAT) return (uint8_t)a;                      /* these two have loaded nothing */
    if (kind == HVQ_TB_IDENTITY) return (uint8_t)lane;
    const uint32_t C = L->cnt[0][lane], N = L->cnt[0][255];
    if (!N) return (uint8_t)lane;
    if (kind == HVQ_TB_EQUALIZE) {
        const uint32_t cmin = L->sel[0], D = N - cmin;
        if (!D) return (uint8_t)lane;
        const uint64_t num = C >= cmin ? C - cmin : 0u;
        return (uint8_t)((510u * num + D) / (2u * (uint64_t)D));
    }
    if (kind == HVQ_TB_STRETCH) {
        const uint32_t lo = L->sel[1], hi = L->sel[2];
        if (hi <= lo) return (uint8_t)lane;
        if (lane <= lo) return 0u;
        if (lane >= hi) return 255u;
        return (uint8_t)((510u * (lane - lo) + (hi - lo)) / (2u * (hi - lo)));
    }
    const uint32_t t = L->valid[0] ? L->t[0] : 0u;                   /* HVQ_TB_OTSU: a single value has no valid candidate */
    return lane > t ? 255u : 0u;
}

#endif
