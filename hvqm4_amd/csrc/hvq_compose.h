/*
 * hvq_compose.h -- what the compose kernel (hvq_compose.hip), the runtime (hvq_compose_pictures) and the tests' fake device share: the
 * rule that chooses a layer-plane's body, the test that lets a tile skip a layer, the index arithmetic of both bodies, the finish, and
 * the records of a target plane and of a layer plane.  Plain C++ that compiles for the host and the device alike.
 * include/hvqm4_amd.h specifies the values.
 *
 * A workgroup of 256 lanes takes HVQ_CP_TW x HVQ_CP_TH = 64 x 16 targets of a plane; lane l owns the dword of columns 4 (l & 15) ..
 * 4 (l & 15) + 3 of row l >> 4 and keeps its four accumulators in registers from the first layer to the store.  No LDS.
 */
#ifndef HVQ_COMPOSE_H
#define HVQ_COMPOSE_H

#include <stdint.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_CP_FN __host__ __device__ static inline
#else
#define HVQ_CP_FN static inline
#endif

/* The choice of the body for a layer plane, all numbers in samples of the plane.  Aligned: the rectangle's x edges in the target (dx,
 * dx + w) are multiples of 4 and source and target columns agree mod 4: every target dword lies wholly inside or wholly outside the
 * rectangle, and the four source bytes of one inside are one aligned dword (the source plane starts 4-byte aligned and its pitch is a
 * multiple of 4).  Anything else is general.  force: every layer plane general (hvq_compose_force_general). */
HVQ_CP_FN uint32_t hvq_cp_body(int32_t sx, int32_t dx, int32_t w, int force)
{
    return !force && ((dx | w | (sx - dx)) & 3) == 0 ? HVQ_CP_ALIGNED : HVQ_CP_GENERAL;
}

/* does the layer's target rectangle miss the tile whose first target is (c0, r0)?  Uniform over a workgroup */
HVQ_CP_FN int hvq_cp_misses(const HvqComposeRec *r, uint32_t c0, uint32_t r0)
{
    return r->dx >= (int32_t)(c0 + HVQ_CP_TW) || r->dx + r->w <= (int32_t)c0 || r->dy >= (int32_t)(r0 + HVQ_CP_TH) || r->dy + r->h <= (int32_t)r0;
}

/* which of the four targets (x .. x + 3, y) the layer covers: bit i for x + i */
HVQ_CP_FN uint32_t hvq_cp_cover(const HvqComposeRec *r, int32_t x, int32_t y)
{
    if (y < r->dy || y >= r->dy + r->h) return 0u;
    uint32_t m = 0;
    for (int32_t i = 0; i < 4; ++i) m |= (x + i >= r->dx && x + i < r->dx + r->w) ? 1u << i : 0u;
    return m;
}

/* the byte of the source plane that lands on target (x, y): inside the plane for every covered target; may be negative or past the
 * plane for one that is not covered */
HVQ_CP_FN int32_t hvq_cp_src_byte(const HvqComposeRec *r, int32_t x, int32_t y)
{
    return (y - r->dy + r->sy) * (int32_t)r->pitch + (x - r->dx + r->sx);
}
/* the dwords of the source plane */
HVQ_CP_FN int32_t hvq_cp_src_dwords(const HvqComposeRec *r) { return (int32_t)((r->pitch >> 2) * r->ny); }

/* the general body's four source bytes, byte `a` first, from the aligned dwords a >> 2 (lo) and (a >> 2) + 1 (hi) */
HVQ_CP_FN uint32_t hvq_cp_funnel(uint32_t lo, uint32_t hi, uint32_t a)
{
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * (a & 3u)));
}

/* a layer's step of one accumulator: PUT is a select */
HVQ_CP_FN int32_t hvq_cp_step(int32_t acc, uint32_t covered, uint32_t put, int32_t weight, uint32_t s)
{
    const int32_t below = put ? 0 : acc;
#if defined(__HIP_DEVICE_COMPILE__)
    return covered ? below + __mul24(weight, (int32_t)s) : acc;      /* |weight| <= 2^22, s <= 255: the 24-bit multiplier is exact */
#else
    return covered ? below + weight * (int32_t)s : acc;
#endif
}

/* the finish: ONE rounding, floor towards minus infinity (an arithmetic shift), then the bias and the clamp */
HVQ_CP_FN uint32_t hvq_cp_finish(int32_t acc, int32_t half, int32_t shift, int32_t bias)
{
    const int32_t v = ((acc + half) >> shift) + bias;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

/* the job of plane p of a target: mx x my its samples */
static inline HvqComposeJob hvq_cp_job(uint64_t dst, uint32_t mx, uint32_t my, uint32_t first, uint32_t count, int32_t shift, int32_t bias, uint32_t plane)
{
    HvqComposeJob j;
    j.dst = dst; j.mx = mx; j.my = my;
    j.tiles_x = (mx + HVQ_CP_TW - 1u) / HVQ_CP_TW;
    j.tiles = j.tiles_x * ((my + HVQ_CP_TH - 1u) / HVQ_CP_TH);
    j.first = first; j.count = count;
    j.shift = shift; j.half = shift ? 1 << (shift - 1) : 0; j.bias = bias;
    j.plane = plane;
    return j;
}

/* the record of one plane of a layer: the source plane (`src`, ny rows of pitch samples) and the layer's rectangles in its samples */
static inline HvqComposeRec hvq_cp_rec(uint64_t src, uint32_t pitch, uint32_t ny, int32_t sx, int32_t sy, int32_t w, int32_t h, int32_t dx, int32_t dy,
                                       int32_t weight, uint32_t mode, int force)
{
    HvqComposeRec r;
    r.src = src; r.pitch = pitch; r.ny = ny;
    r.sx = sx; r.sy = sy; r.dx = dx; r.dy = dy; r.w = w; r.h = h;
    r.weight = weight; r.mode = mode;
    r.body = hvq_cp_body(sx, dx, w, force);
    r.pad[0] = r.pad[1] = r.pad[2] = 0;
    return r;
}

#endif
