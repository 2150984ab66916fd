/*
 * hvq_filter.h -- what the filter kernel (hvq_filter.hip), the runtime (hvq_filter_pictures) and the tests' fake device share: the index
 * arithmetic of a tile (which source row and dword a staged dword is, which staged byte a tap meets), the combination and the one
 * rounding, the choice of the body and the job record of a plane.  Plain C++ that compiles for the host and the device alike.
 * include/hvqm4_amd.h specifies the values.
 */
#ifndef HVQ_FILTER_H
#define HVQ_FILTER_H

#include <stdint.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_FL_FN __host__ __device__ static inline
#else
#define HVQ_FL_FN static inline
#endif

/* The staged rows of the tile whose first target row is r0: staged row rr, 0 <= rr < HVQ_FL_TH + 2 rmax, is source row
 * r0 + rr - rmax clamped into the plane (the border replicates the edge sample: rows are clamped when staging). */
HVQ_FL_FN uint32_t hvq_fl_stage_row(uint32_t r0, uint32_t rr, uint32_t rmax, uint32_t ny)
{
    const int32_t y = (int32_t)(r0 + rr) - (int32_t)rmax;
    return y < 0 ? 0u : y >= (int32_t)ny ? ny - 1u : (uint32_t)y;
}
/* A staged row is HVQ_FL_ROW_DWORDS aligned dwords: the source bytes c0 - HVQ_FL_HALO .. c0 + HVQ_FL_TW + HVQ_FL_HALO - 1 (c0, the
 * tile's first column, is a multiple of HVQ_FL_TW).  Dword k of it is the row's dword c0 / 4 - HVQ_FL_HALO / 4 + k; one that lies
 * outside the row is replaced by the nearest inside (its bytes are never looked at: columns are clamped when reading). */
HVQ_FL_FN uint32_t hvq_fl_stage_dword(uint32_t c0, uint32_t k, uint32_t nx)
{
    const int32_t d = (int32_t)(c0 >> 2) - (int32_t)(HVQ_FL_HALO >> 2) + (int32_t)k, last = (int32_t)(nx >> 2) - 1;
    return d < 0 ? 0u : d > last ? (uint32_t)last : (uint32_t)d;
}
/* The byte of a staged row that tap i of a term of radius rx meets for target column c (c0 <= c < c0 + HVQ_FL_TW): source column
 * c + i - rx clamped into the row, counted from the first staged byte.  With min(c, nx - 1) for the lanes past the plane the result
 * lies in [0, 4 HVQ_FL_ROW_DWORDS): x >= max(c0 - rx, 0) >= c0 - HVQ_FL_HALO and x <= c + rx < c0 + HVQ_FL_TW + HVQ_FL_HALO. */
HVQ_FL_FN uint32_t hvq_fl_tap_byte(uint32_t c0, uint32_t c, uint32_t i, uint32_t rx, uint32_t nx)
{
    const int32_t cc = (int32_t)(c < nx ? c : nx - 1u);
    int32_t x = cc + (int32_t)i - (int32_t)rx;
    x = x < 0 ? 0 : x >= (int32_t)nx ? (int32_t)nx - 1 : x;
    return (uint32_t)(x - (int32_t)c0 + (int32_t)HVQ_FL_HALO);
}
/* S = combine(T0, T1); out = min(255, max(0, floor((S + half) / 2^shift) + bias)): the floor is an arithmetic shift, one rounding.
 * |S| + half < 2^31 (the gain is at most 2^22). */
HVQ_FL_FN uint32_t hvq_fl_finish(int32_t t0, int32_t t1, int32_t combine, int32_t half, int32_t shift, int32_t bias)
{
    int32_t s = t0 + t1;
    if (combine == 1) s = s < 0 ? -s : s;
    else if (combine == 2) s = (t0 < 0 ? -t0 : t0) + (t1 < 0 ? -t1 : t1);
    const int32_t v = ((s + half) >> shift) + bias;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

/* a plane filter that leaves every sample as it is: one term of radius 0 whose weight is 2^shift, no bias (a sample is never
 * negative: any combine) */
static inline int hvq_fl_is_identity(const HvqFilterPlaneDev *f)
{
    return f->terms == 1 && f->term[0].rx == 0 && f->term[0].ry == 0 && f->bias == 0 && f->term[0].wx[0] * f->term[0].wy[0] == (1 << f->shift);
}

/* the job of a plane; copy: the plane's filter is the identity and the copy body is not switched off (hvq_filter_force_filter) */
static inline HvqFilterJob hvq_fl_job(uint64_t src, uint64_t dst, uint32_t nx, uint32_t ny, uint32_t pf, int copy)
{
    HvqFilterJob j;
    j.src = src; j.dst = dst; j.nx = nx; j.ny = ny; j.pf = pf;
    j.body = copy ? HVQ_FL_COPY : HVQ_FL_FILTER;
    const uint32_t tw = copy ? HVQ_FL_CTW : HVQ_FL_TW, th = copy ? HVQ_FL_CTH : HVQ_FL_TH;
    j.tiles_x = (nx + tw - 1u) / tw;
    j.tiles = j.tiles_x * ((ny + th - 1u) / th);
    j.pad[0] = j.pad[1] = 0;
    return j;
}

#endif
