/*
 * hvq_label.h -- what the label and select kernels (hvq_label.hip), the runtime (hvq_label_pictures, hvq_select_components) and the
 * tests' fake device share: the job records, the index arithmetic of a tile, a seam item and a chunk, the union and find steps, the
 * numbering of the roots and the record arithmetic, written per lane: a kernel calls a phase with its lane and puts a barrier behind it
 * where one is needed, the fake device calls it for every lane in turn.  C++ that compiles for the host and the device alike: integers
 * only.  include/hvqm4_amd.h specifies the values.
 *
 * The map is the parent array.  An entry is 0 for background, otherwise parent's raster index + 1; a root is its own parent.  A union
 * links the root of the LARGER index to the smaller one, so a parent's index is below its child's everywhere and always: no cycle can
 * form, a walk towards a root strictly descends, and a component's root is its first sample.  That is also what bounds every loop here:
 * a walk from index a takes at most a steps; a union from (a, b) descends in a or in b in every round that does not end it, so it takes
 * fewer than a + b + 2 rounds.  A lane that nevertheless uses up its budget -- memory that something else overwrote -- reports it and
 * leaves (status HVQ_LBL_INCOMPLETE).
 *
 * Atomic steps.  A union is lock-free: find both roots, atomic-min the larger root's entry with the smaller root + 1; when the entry was
 * no root any more (another lane linked it meanwhile) the union goes on with the entry's former parent, which the min may have cut off.
 * A retry follows another lane's progress; nobody waits.  HVQ_LB_PLAIN (the fake device, one lane after the other) turns the atomic
 * steps into plain ones.
 */
#ifndef HVQ_LABEL_H
#define HVQ_LABEL_H

#include <stdint.h>

#include "hvq_desc.h"

#define HVQ_LB_INCOMPLETE 1u                                          /* HVQ_LBL_INCOMPLETE of include/hvqm4_amd.h */

/* ------------------------------------------------------------------------------------------------ the jobs (host) */
static inline HvqLabelJob hvq_lb_job(uint64_t src, uint64_t labels, uint64_t comps, uint32_t nx, uint32_t ny, uint32_t lo, uint32_t hi,
                                     uint32_t conn, uint32_t cap)
{
    HvqLabelJob j;
    j.src = src; j.labels = labels; j.comps = comps;
    j.nx = nx; j.ny = ny;                                            /* nx is a multiple of 4 */
    j.tx = (nx + HVQ_LB_TX - 1u) / HVQ_LB_TX;
    j.ty = (ny + HVQ_LB_TY - 1u) / HVQ_LB_TY;
    j.seams = (j.ty - 1u) * nx + (j.tx - 1u) * ny;
    j.chunks = (nx * ny + HVQ_LB_CHUNK - 1u) / HVQ_LB_CHUNK;
    j.lo = lo; j.hi = hi; j.conn = conn; j.cap = cap;
    return j;
}

static inline HvqSelectJob hvq_sl_job(uint64_t labels, uint64_t comps, uint64_t dst, uint32_t nx, uint32_t ny, uint32_t cap, int select,
                                      const uint32_t range[6], uint32_t invert)
{
    HvqSelectJob j;
    j.labels = select ? labels : 0u; j.comps = select ? comps : 0u; j.dst = dst;
    j.dwords = (nx >> 2) * ny;
    j.tiles = (j.dwords + HVQ_MP_TILE - 1u) / HVQ_MP_TILE;
    j.body = select ? HVQ_SL_SELECT : HVQ_SL_FILL;
    j.cap = select ? cap : 0u;
    j.area_min = select ? range[0] : 0u; j.area_max = select ? range[1] : 0u;
    j.w_min = select ? range[2] : 0u; j.w_max = select ? range[3] : 0u;
    j.h_min = select ? range[4] : 0u; j.h_max = select ? range[5] : 0u;
    j.invert = select ? invert : 0u;
    j.pad[0] = j.pad[1] = j.pad[2] = 0u;
    return j;
}

/* ------------------------------------------------------------------------------------------------ the lanes' code */
#if defined(HVQ_LB_PLAIN) || defined(__HIPCC__)

#if defined(HVQ_LB_PLAIN)
#define HVQ_LB_FN static inline
#define HVQ_LB_UNROLL
#define HVQ_LB_WG    0
#define HVQ_LB_AGENT 1
#define HVQ_LB_LOAD(p, scope) (*(p))
static inline uint32_t hvq_lb_plain_min(uint32_t *p, uint32_t v) { const uint32_t o = *p; if (v < o) *p = v; return o; }
#define HVQ_LB_MIN(p, v, scope) hvq_lb_plain_min((p), (v))
#define HVQ_LB_ADD64(p, v) (void)(*(p) += (v))
#define HVQ_LB_MIN64(p, v) (void)(*(p) = (v) < *(p) ? (v) : *(p))
#define HVQ_LB_MAX64(p, v) (void)(*(p) = (v) > *(p) ? (v) : *(p))
#else
#define HVQ_LB_FN __device__ static inline __attribute__((always_inline))
#define HVQ_LB_UNROLL _Pragma("unroll")
#define HVQ_LB_WG    __HIP_MEMORY_SCOPE_WORKGROUP
#define HVQ_LB_AGENT __HIP_MEMORY_SCOPE_AGENT
#define HVQ_LB_LOAD(p, scope) __hip_atomic_load((p), __ATOMIC_RELAXED, scope)
#define HVQ_LB_MIN(p, v, scope) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, scope)
#define HVQ_LB_ADD64(p, v) (void)__hip_atomic_fetch_add((p), (uint64_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define HVQ_LB_MIN64(p, v) (void)__hip_atomic_fetch_min((p), (uint64_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define HVQ_LB_MAX64(p, v) (void)__hip_atomic_fetch_max((p), (uint64_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

/* sixteen bytes of the map: four entries of a row (nx is a multiple of 4 and the map a multiple of 16) */
typedef struct __attribute__((aligned(16))) HvqLbQuad { uint32_t v[4]; } HvqLbQuad;

HVQ_LB_FN uint32_t hvq_lb_samples(const HvqLabelJob &J) { return J.nx * J.ny; }

/* a and b, foreground entries of P, become one class -> 0 when the budget ran out */
template <int SCOPE>
HVQ_LB_FN uint32_t hvq_lb_union(uint32_t *P, uint32_t a, uint32_t b, uint32_t budget)
{
    while (budget--) {
        const uint32_t pa = HVQ_LB_LOAD(P + a, SCOPE) - 1u;
        if (pa < a) { a = pa; continue; }
        const uint32_t pb = HVQ_LB_LOAD(P + b, SCOPE) - 1u;
        if (pb < b) { b = pb; continue; }
        if (a == b) return 1u;
        if (pa != a || pb != b) return 0u;                           /* an entry above its own index: not ours */
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = HVQ_LB_MIN(P + hi, lo + 1u, SCOPE) - 1u;
        if (old == hi) return 1u;
        if (old > hi) return 0u;
        a = old; b = lo;                                              /* hi was linked meanwhile: its former parent joins lo */
    }
    return 0u;
}

/* the root of foreground entry a -> its index, or ~0 when the budget ran out */
template <int SCOPE>
HVQ_LB_FN uint32_t hvq_lb_find(const uint32_t *P, uint32_t a, uint32_t budget)
{
    while (budget--) {
        const uint32_t p = HVQ_LB_LOAD(P + a, SCOPE) - 1u;
        if (p == a) return a;
        if (p > a) return ~0u;
        a = p;
    }
    return ~0u;
}

/* ---- launch 1: a tile in LDS.  Lane l holds the entries 4 l .. 4 l + 3 of P[HVQ_LB_TILE]: row l / 16, columns 4 (l % 16) .. */
HVQ_LB_FN int hvq_lb_tile_at(const HvqLabelJob &J, uint32_t tile, uint32_t lane, uint32_t *x, uint32_t *y)
{
    *x = (tile % J.tx) * HVQ_LB_TX + (lane & 15u) * 4u;
    *y = (tile / J.tx) * HVQ_LB_TY + (lane >> 4);
    return *x < J.nx && *y < J.ny;
}

/* the lane's four entries: 0, or the local index + 1 of the start of the run inside the dword */
HVQ_LB_FN void hvq_lb_tile_load(const HvqLabelJob &J, uint32_t tile, uint32_t lane, uint32_t *P)
{
    uint32_t x, y, v = 0u, start = 0u, prev = 0u;
    const int in = hvq_lb_tile_at(J, tile, lane, &x, &y);
    if (in) v = ((const uint32_t *)(uintptr_t)J.src)[(y * J.nx + x) >> 2];
    HVQ_LB_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint32_t a = (v >> (8u * s)) & 255u, l = lane * 4u + s;
        const uint32_t fg = in && a >= J.lo && a <= J.hi ? 1u : 0u;
        if (fg && !prev) start = l;
        P[l] = fg ? start + 1u : 0u;
        prev = fg;
    }
}

/* the lane's entries join their neighbours to the left and above inside the tile -> 0 when a budget ran out */
HVQ_LB_FN uint32_t hvq_lb_tile_merge(const HvqLabelJob &J, uint32_t lane, uint32_t *P)
{
    const uint32_t lx0 = (lane & 15u) * 4u, ly = lane >> 4, budget = 2u * HVQ_LB_TILE + 2u;
    uint32_t ok = 1u;
    HVQ_LB_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint32_t l = lane * 4u + s, lx = lx0 + s;
        if (!HVQ_LB_LOAD(P + l, HVQ_LB_WG)) continue;
        if (s == 0u && lx > 0u && HVQ_LB_LOAD(P + l - 1u, HVQ_LB_WG)) ok &= hvq_lb_union<HVQ_LB_WG>(P, l, l - 1u, budget);
        if (!ly) continue;
        if (HVQ_LB_LOAD(P + l - HVQ_LB_TX, HVQ_LB_WG)) {
            /* left and above-left both foreground: this sample joins the left one, that one the one above it (by this rule, or by its
             * own union: column 0 of the tile has no left), and above-left and above lie in one row: nothing to add */
            if (lx > 0u && HVQ_LB_LOAD(P + l - 1u, HVQ_LB_WG) && HVQ_LB_LOAD(P + l - HVQ_LB_TX - 1u, HVQ_LB_WG)) continue;
            ok &= hvq_lb_union<HVQ_LB_WG>(P, l, l - HVQ_LB_TX, budget);
            continue;
        }
        if (J.conn != 8u) continue;                                  /* the diagonals count only where the sample above is background */
        if (lx > 0u && HVQ_LB_LOAD(P + l - HVQ_LB_TX - 1u, HVQ_LB_WG)) ok &= hvq_lb_union<HVQ_LB_WG>(P, l, l - HVQ_LB_TX - 1u, budget);
        if (lx + 1u < HVQ_LB_TX && HVQ_LB_LOAD(P + l - HVQ_LB_TX + 1u, HVQ_LB_WG)) ok &= hvq_lb_union<HVQ_LB_WG>(P, l, l - HVQ_LB_TX + 1u, budget);
    }
    return ok;
}

/* the lane's four entries of the map: 0, or the raster index + 1 of the root in the plane -> 0 when a budget ran out */
HVQ_LB_FN uint32_t hvq_lb_tile_store(const HvqLabelJob &J, uint32_t tile, uint32_t lane, const uint32_t *P)
{
    uint32_t x, y, ok = 1u;
    if (!hvq_lb_tile_at(J, tile, lane, &x, &y)) return 1u;
    const uint32_t x0 = x - (lane & 15u) * 4u, y0 = y - (lane >> 4);
    HvqLbQuad q;
    HVQ_LB_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint32_t l = lane * 4u + s;
        q.v[s] = 0u;
        if (!P[l]) continue;
        const uint32_t r = hvq_lb_find<HVQ_LB_WG>(P, l, HVQ_LB_TILE + 1u);
        if (r >= HVQ_LB_TILE) { ok = 0u; q.v[s] = (y * J.nx + x + s) + 1u; continue; }     /* a class of its own: the map stays a forest */
        q.v[s] = (y0 + r / HVQ_LB_TX) * J.nx + x0 + r % HVQ_LB_TX + 1u;
    }
    *(HvqLbQuad *)((uint32_t *)(uintptr_t)J.labels + (y * J.nx + x)) = q;
    return ok;
}

/* ---- launch 2: a seam item.  Items 0 .. (ty - 1) nx - 1 are the samples of the upper rows of the tile rows 1 .., the rest those of the
 * left columns of the tile columns 1 ..; each joins its neighbours across the seam.  Every access of the map is an agent-scope atomic. */
HVQ_LB_FN uint32_t hvq_lb_seam(const HvqLabelJob &J, uint32_t item)
{
    if (item >= J.seams) return 1u;
    uint32_t *L = (uint32_t *)(uintptr_t)J.labels;
    const uint32_t nx = J.nx, ny = J.ny, across = (J.ty - 1u) * nx, budget = 2u * nx * ny + 2u;
    uint32_t ok = 1u;
    if (item < across) {
        const uint32_t x = item % nx, y = (item / nx + 1u) * HVQ_LB_TY, i = y * nx + x;      /* y <= (ty - 1) TY < ny */
        if (!HVQ_LB_LOAD(L + i, HVQ_LB_AGENT)) return 1u;
        if (HVQ_LB_LOAD(L + i - nx, HVQ_LB_AGENT)) return hvq_lb_union<HVQ_LB_AGENT>(L, i, i - nx, budget);
        if (J.conn != 8u) return 1u;
        if (x > 0u && HVQ_LB_LOAD(L + i - nx - 1u, HVQ_LB_AGENT)) ok &= hvq_lb_union<HVQ_LB_AGENT>(L, i, i - nx - 1u, budget);
        if (x + 1u < nx && HVQ_LB_LOAD(L + i - nx + 1u, HVQ_LB_AGENT)) ok &= hvq_lb_union<HVQ_LB_AGENT>(L, i, i - nx + 1u, budget);
    } else {
        const uint32_t it = item - across, y = it % ny, x = (it / ny + 1u) * HVQ_LB_TX, i = y * nx + x;   /* x <= (tx - 1) TX < nx */
        if (!HVQ_LB_LOAD(L + i, HVQ_LB_AGENT)) return 1u;
        if (HVQ_LB_LOAD(L + i - 1u, HVQ_LB_AGENT)) return hvq_lb_union<HVQ_LB_AGENT>(L, i, i - 1u, budget);
        if (J.conn != 8u) return 1u;
        if (y > 0u && HVQ_LB_LOAD(L + i - nx - 1u, HVQ_LB_AGENT)) ok &= hvq_lb_union<HVQ_LB_AGENT>(L, i, i - nx - 1u, budget);
        if (y + 1u < ny && HVQ_LB_LOAD(L + i + nx - 1u, HVQ_LB_AGENT)) ok &= hvq_lb_union<HVQ_LB_AGENT>(L, i, i + nx - 1u, budget);
    }
    return ok;
}

/* ---- launch 3: the roots of the tiles that a seam union linked point at their roots in the plane.  Such an entry's parent lies in
 * another tile (an entry whose parent lies in its own tile is left alone: nearly all are ordinary samples under their tile's root), so
 * the walks of launch 5 are two or three steps.  Only the depth of the forest changes: a lane that reads an entry before or after this
 * store reads an ancestor either way -> 0 when a budget ran out */
HVQ_LB_FN uint32_t hvq_lb_flatten(const HvqLabelJob &J, uint32_t chunk, uint32_t lane)
{
    uint32_t *L = (uint32_t *)(uintptr_t)J.labels;
    const uint32_t N = hvq_lb_samples(J), i = chunk * HVQ_LB_CHUNK + lane * 4u;
    uint32_t ok = 1u;
    if (i >= N) return 1u;
    const uint32_t y = i / J.nx, x = i % J.nx;
    const HvqLbQuad e = *(const HvqLbQuad *)(L + i);
    HVQ_LB_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint32_t v = e.v[s];
        if (!v || v - 1u >= i + s) continue;                          /* background, or a root */
        const uint32_t p = v - 1u, py = p / J.nx, px = p - py * J.nx;
        if (py / HVQ_LB_TY == y / HVQ_LB_TY && px / HVQ_LB_TX == (x + s) / HVQ_LB_TX) continue;
        const uint32_t r = hvq_lb_find<HVQ_LB_AGENT>(L, p, p + 2u);
        if (r > p) { ok = 0u; continue; }
        if (r != p) L[i + s] = r + 1u;
    }
    return ok;
}

/* ---- launch 4: ONE workgroup a picture numbers the roots in raster order, HVQ_LB_SPAN samples a round, sixteen consecutive ones a lane.
 * -> the mask of the lane's roots in this round; *fg grows by its foreground samples */
HVQ_LB_FN uint32_t hvq_lb_number_count(const HvqLabelJob &J, uint32_t round, uint32_t lane, uint32_t *fg)
{
    const uint32_t *L = (const uint32_t *)(uintptr_t)J.labels;
    const uint32_t N = hvq_lb_samples(J), i0 = round * HVQ_LB_SPAN + lane * 16u;
    uint32_t mask = 0u;
    HVQ_LB_UNROLL
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t i = i0 + 4u * q;
        if (i >= N) continue;                                         /* N is a multiple of 4 */
        const HvqLbQuad e = *(const HvqLbQuad *)(L + i);
        HVQ_LB_UNROLL
        for (uint32_t s = 0; s < 4u; ++s) {
            if (e.v[s]) ++*fg;
            if (e.v[s] == i + s + 1u) mask |= 1u << (4u * q + s);
        }
    }
    return mask;
}

/* the lane's roots get the numbers before + 1 ..: into the map (HVQ_LB_NUMBERED) and, up to cap, as a fresh record */
HVQ_LB_FN void hvq_lb_number_store(const HvqLabelJob &J, uint32_t round, uint32_t lane, uint32_t mask, uint32_t before)
{
    uint32_t *L = (uint32_t *)(uintptr_t)J.labels;
    uint64_t *C = (uint64_t *)(uintptr_t)J.comps;
    const uint32_t i0 = round * HVQ_LB_SPAN + lane * 16u;
    uint32_t k = before;
    for (; mask; mask &= mask - 1u) {
        const uint32_t i = i0 + (uint32_t)__builtin_ctz(mask);
        ++k;
        L[i] = HVQ_LB_NUMBERED | k;
        if (k > J.cap) continue;
        uint64_t *row = C + 8u * (uint64_t)k;
        row[0] = 0u; row[1] = 0xffffffffu; row[2] = 0xffffffffu; row[3] = 0u; row[4] = 0u; row[5] = i; row[6] = 0u; row[7] = 0u;
    }
}

/* row 0: launch 0 zeroes it, the lanes of the launches store their status there, one lane of launch 4 the counts */
HVQ_LB_FN void hvq_lb_head_begin(const HvqLabelJob &J)
{
    uint64_t *C = (uint64_t *)(uintptr_t)J.comps;
    for (uint32_t m = 0; m < 8u; ++m) C[m] = 0u;
}
HVQ_LB_FN void hvq_lb_head_status(const HvqLabelJob &J) { ((uint64_t *)(uintptr_t)J.comps)[3] = HVQ_LB_INCOMPLETE; }
HVQ_LB_FN void hvq_lb_head_counts(const HvqLabelJob &J, uint32_t K, uint32_t F)
{
    uint64_t *C = (uint64_t *)(uintptr_t)J.comps;
    C[0] = K; C[1] = K < J.cap ? K : J.cap; C[2] = F;
}

/* ---- launch 5: every entry becomes its component's number (still HVQ_LB_NUMBERED: a walk of another lane may pass through it), and the
 * records gather.  What a lane adds to ONE record: */
typedef struct HvqLbRec { uint32_t k, x0, y0, x1, y1; uint64_t area, sx, sy; } HvqLbRec;

HVQ_LB_FN void hvq_lb_rec_none(HvqLbRec *R) { R->k = 0u; R->x0 = R->y0 = 0xffffffffu; R->x1 = R->y1 = 0u; R->area = R->sx = R->sy = 0u; }
HVQ_LB_FN void hvq_lb_rec_add(HvqLbRec *R, uint32_t x, uint32_t y)
{
    R->x0 = x < R->x0 ? x : R->x0; R->y0 = y < R->y0 ? y : R->y0;
    R->x1 = x > R->x1 ? x : R->x1; R->y1 = y > R->y1 ? y : R->y1;
    R->area += 1u; R->sx += x; R->sy += y;
}
HVQ_LB_FN void hvq_lb_rec_flush(const HvqLabelJob &J, uint32_t stored, const HvqLbRec *R)
{
    if (!R->k || R->k > stored || R->k > J.cap) return;
    uint64_t *row = (uint64_t *)(uintptr_t)J.comps + 8u * (uint64_t)R->k;
    HVQ_LB_ADD64(row + 0, R->area);
    HVQ_LB_MIN64(row + 1, R->x0); HVQ_LB_MIN64(row + 2, R->y0);
    HVQ_LB_MAX64(row + 3, R->x1); HVQ_LB_MAX64(row + 4, R->y1);
    HVQ_LB_ADD64(row + 6, R->sx); HVQ_LB_ADD64(row + 7, R->sy);
}

/* the lane's four entries of chunk `chunk`.  All runs but the last are flushed here; the last is left in *last (k 0: none) for the
 * caller, which may first add up the lanes of a wave that share a number -> 0 when a budget ran out */
HVQ_LB_FN uint32_t hvq_lb_resolve(const HvqLabelJob &J, uint32_t chunk, uint32_t lane, uint32_t stored, HvqLbRec *last)
{
    uint32_t *L = (uint32_t *)(uintptr_t)J.labels;
    const uint32_t N = hvq_lb_samples(J), i = chunk * HVQ_LB_CHUNK + lane * 4u;
    uint32_t ok = 1u;
    hvq_lb_rec_none(last);
    if (i >= N) return 1u;
    const uint32_t y = i / J.nx, x = i % J.nx;
    HvqLbQuad e = *(const HvqLbQuad *)(L + i);
    HVQ_LB_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) {
        uint32_t v = e.v[s], k = 0u;
        if (v & HVQ_LB_NUMBERED) k = v & ~HVQ_LB_NUMBERED;
        else if (v) {
            uint32_t p = v - 1u, budget = i + s + 2u;                 /* p <= i + s, and every step descends */
            for (; budget; --budget) {
                if (p >= N) break;
                const uint32_t w = HVQ_LB_LOAD(L + p, HVQ_LB_AGENT);
                if (w & HVQ_LB_NUMBERED) { k = w & ~HVQ_LB_NUMBERED; break; }
                if (!w || w - 1u >= p) break;
                p = w - 1u;
            }
            if (!k) ok = 0u;
        }
        e.v[s] = k ? HVQ_LB_NUMBERED | k : 0u;
        if (k != last->k) {
            hvq_lb_rec_flush(J, stored, last);
            hvq_lb_rec_none(last);
            last->k = k;
        }
        if (k) hvq_lb_rec_add(last, x + s, y);
    }
    *(HvqLbQuad *)(L + i) = e;
    return ok;
}

/* ---- launch 6: the mark leaves */
HVQ_LB_FN void hvq_lb_finish(const HvqLabelJob &J, uint32_t chunk, uint32_t lane)
{
    uint32_t *L = (uint32_t *)(uintptr_t)J.labels;
    const uint32_t i = chunk * HVQ_LB_CHUNK + lane * 4u;
    if (i >= hvq_lb_samples(J)) return;
    HvqLbQuad e = *(const HvqLbQuad *)(L + i);
    HVQ_LB_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) e.v[s] &= ~HVQ_LB_NUMBERED;
    *(HvqLbQuad *)(L + i) = e;
}

/* ---- select: the four samples of dword d of the Y plane */
HVQ_LB_FN uint32_t hvq_sl_dword(const HvqSelectJob &J, uint32_t stored, uint32_t d)
{
    const uint64_t *C = (const uint64_t *)(uintptr_t)J.comps;
    const HvqLbQuad e = *(const HvqLbQuad *)((const uint32_t *)(uintptr_t)J.labels + 4u * (uint64_t)d);
    uint32_t out = 0u;
    HVQ_LB_UNROLL
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint32_t k = e.v[s];
        uint32_t sel = 0u;
        if (k >= 1u && k <= stored && k <= J.cap) {
            const uint64_t *row = C + 8u * (uint64_t)k;
            const uint64_t area = row[0], w = row[3] - row[1] + 1u, h = row[4] - row[2] + 1u;
            sel = area >= J.area_min && area <= J.area_max && w >= J.w_min && w <= J.w_max && h >= J.h_min && h <= J.h_max ? 1u : 0u;
        }
        out |= ((sel ^ J.invert) & 1u ? 255u : 0u) << (8u * s);
    }
    return out;
}

#endif
#endif
