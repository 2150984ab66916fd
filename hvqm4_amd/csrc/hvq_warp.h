/*
 * hvq_warp.h -- what the warp kernel (hvq_warp.hip), the runtime (hvq_warp_pictures) and the tests' fake device share: the coordinate
 * arithmetic of a target sample, the source bounding box of a tile, the border rule, the finish, the job record of a plane and the
 * choice of the body.  Plain C++ that compiles for the host and the device alike.  include/hvqm4_amd.h specifies the values.
 *
 * Tile and LDS budget.  A workgroup of 256 lanes takes HVQ_WP_TW x HVQ_WP_TH = 64 x 16 targets of a plane; lane (column c, wave g)
 * computes the targets (c, 4 g .. 4 g + 3), the tile's 1024 bytes meet in LDS (1 KiB) and every lane stores one dword.  The tiled body
 * stages the tile's source box into HVQ_WP_LDS_DWORDS = 4096 dwords (16 KiB): a plane whose box needs more takes the direct body.
 */
#ifndef HVQ_WARP_H
#define HVQ_WARP_H

#include <stdint.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_WP_FN __host__ __device__ static inline
#else
#define HVQ_WP_FN static inline
#endif

/* U8 (or V8) from NU (NV): floor((NU + 256 h) / (512 h)) as an arithmetic shift by s = 8 + h, saturated to [-512, 256 n].  The
 * saturation changes no value: at or below -512 both taps lie left of the plane with whatever weights, at 256 n both lie right of it,
 * and outside the plane every tap is the same sample (REPLICATE) or the fill (CONSTANT).  What comes back fits 23 bits. */
HVQ_WP_FN int32_t hvq_wp_u8(int64_t nu, uint32_t s, uint32_t n)
{
    const int64_t u = (nu + ((int64_t)1 << (s - 1u))) >> s;
    const int64_t hi = (int64_t)256 * n;
    return (int32_t)(u < -512 ? -512 : u > hi ? hi : u);
}
HVQ_WP_FN int32_t hvq_wp_clamp(int32_t v, uint32_t n) { return v < 0 ? 0 : v >= (int32_t)n ? (int32_t)n - 1 : v; }

/* S from the four taps and the two fractions (0 .. 255), then ONE rounding: S + 32768 <= 65536 * 255 + 32768 < 2^31 */
HVQ_WP_FN uint32_t hvq_wp_finish(uint32_t fx, uint32_t fy, uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11)
{
    const uint32_t s = (256u - fy) * ((256u - fx) * t00 + fx * t01) + fy * ((256u - fx) * t10 + fx * t11);
    return (s + 32768u) >> 16;
}

/* the source bounding box of the tile whose first target is (c0, r0): the columns x0 .. x1 and rows y0 .. y1 (inclusive, inside the
 * plane) that hold every tap of every target of the tile after the border rule's clamp.  NU is affine in the target, the shift and
 * the saturation are monotone: the extremes are met at the tile's four corners (of the whole tile, also where it leaves the plane). */
typedef struct HvqWarpBox { int32_t x0, x1, y0, y1; } HvqWarpBox;
HVQ_WP_FN void hvq_wp_range(int64_t c, int32_t a, int32_t b, uint32_t c0, uint32_t r0, uint32_t s, uint32_t n, int32_t *lo, int32_t *hi)
{
    const int64_t o = c + (int64_t)a * c0 + (int64_t)b * r0;
    const int64_t da = (int64_t)a * (HVQ_WP_TW - 1u), db = (int64_t)b * (HVQ_WP_TH - 1u);
    const int32_t u0 = hvq_wp_u8(o, s, n), u1 = hvq_wp_u8(o + da, s, n), u2 = hvq_wp_u8(o + db, s, n), u3 = hvq_wp_u8(o + da + db, s, n);
    const int32_t mn = (u0 < u1 ? u0 : u1) < (u2 < u3 ? u2 : u3) ? (u0 < u1 ? u0 : u1) : (u2 < u3 ? u2 : u3);
    const int32_t mx = (u0 > u1 ? u0 : u1) > (u2 > u3 ? u2 : u3) ? (u0 > u1 ? u0 : u1) : (u2 > u3 ? u2 : u3);
    *lo = hvq_wp_clamp(mn >> 8, n);
    *hi = hvq_wp_clamp((mx >> 8) + 1, n);
}
HVQ_WP_FN HvqWarpBox hvq_wp_box(const HvqWarpJob *J, uint32_t c0, uint32_t r0)
{
    HvqWarpBox B;
    hvq_wp_range(J->cu, J->au, J->bu, c0, r0, J->su, J->nx, &B.x0, &B.x1);
    hvq_wp_range(J->cv, J->av, J->bv, c0, r0, J->sv, J->ny, &B.y0, &B.y1);
    return B;
}
/* staged dword idx of a box: row idx / pitch of the box (source row y0 + that), dword idx % pitch of it (the row's dword (x0 >> 2) +
 * that); exact for idx * pitch < 2^32 */
HVQ_WP_FN uint32_t hvq_wp_stage_row(uint32_t idx, uint32_t pitch_mul) { return (uint32_t)(((uint64_t)idx * pitch_mul) >> 32); }
/* the byte of the staged box that holds sample (x, y) of the plane, x0 <= x <= x1, y0 <= y <= y1 */
HVQ_WP_FN uint32_t hvq_wp_lds_byte(const HvqWarpBox *B, uint32_t pitch, int32_t x, int32_t y)
{
    return (uint32_t)(y - B->y0) * pitch * 4u + (uint32_t)(x - (B->x0 & ~3));
}

/* the most samples along one axis that the boxes of a plane's tiles span: two values of NU that lie d apart give U8 that lie at most
 * ceil(d / 2^s) apart, those ix that lie at most ceil(that / 256) apart; one more for the second tap, one more for the count */
HVQ_WP_FN uint32_t hvq_wp_span(int32_t a, int32_t b, uint32_t s, uint32_t n)
{
    const uint64_t d = (uint64_t)(a < 0 ? -(int64_t)a : a) * (HVQ_WP_TW - 1u) + (uint64_t)(b < 0 ? -(int64_t)b : b) * (HVQ_WP_TH - 1u);
    const uint64_t u = (d + ((uint64_t)1 << s) - 1u) >> s;
    const uint64_t span = ((u + 255u) >> 8) + 2u;
    return span < n ? (uint32_t)span : n;
}

/* The choice of the body for a plane whose job is otherwise filled in.  The tiled body needs the box in LDS.  Among the maps it can
 * serve it is taken where a row of 64 adjacent targets crosses at least HVQ_WP_TILED_ROWS source rows (|av| * 63 >= that many rows):
 * there every lane of a direct load meets another cache line, and the staged box turns them into row reads.  Below that the direct
 * body's loads of a wave fall into few lines and the staging is pure overhead (tools/warp_bench.py measures both). */
#define HVQ_WP_TILED_ROWS 8u
HVQ_WP_FN uint32_t hvq_wp_choose(HvqWarpJob *j, int force)
{
    const uint32_t cols = hvq_wp_span(j->au, j->bu, j->su, j->nx), rows = hvq_wp_span(j->av, j->bv, j->sv, j->ny);
    uint32_t pitch = ((cols + 6u) >> 2) | 1u;                        /* a run of `cols` bytes touches (cols + 6) / 4 aligned dwords at the most */
    if (pitch < 3u) pitch = 3u;
    j->pitch = pitch; j->rows = rows;
    j->pitch_mul = (uint32_t)((((uint64_t)1 << 32) / pitch) + 1u);
    const int fits = (uint64_t)pitch * rows <= HVQ_WP_LDS_DWORDS;
    const uint64_t crossed = ((uint64_t)(j->av < 0 ? -(int64_t)j->av : j->av) * (HVQ_WP_TW - 1u)) >> (j->sv + 8u);
    const int wanted = force == 2 || (force == 0 && crossed >= HVQ_WP_TILED_ROWS);
    j->body = fits && wanted ? HVQ_WP_TILED : HVQ_WP_DIRECT;
    return j->body;
}

/* the job of plane p (0: Y) of a picture: m = {m00, m01, m10, m11, t0, t1} of the HvqWarp; (dh, dv) the TARGET sampling of the plane
 * and (sh, sv) the SOURCE sampling of it, both (1, 1) for Y; force: 0 the chosen body, 1 the direct one, 2 the tiled one wherever LDS
 * holds the box */
static inline HvqWarpJob hvq_wp_job(uint64_t src, uint64_t dst, uint32_t nx, uint32_t ny, uint32_t mx, uint32_t my, const int32_t *m, int32_t border, uint32_t fill,
                                    int32_t dh, int32_t dv, int32_t sh, int32_t sv, int force)
{
    HvqWarpJob j;
    j.src = src; j.dst = dst; j.nx = nx; j.ny = ny; j.mx = mx; j.my = my;
    j.au = 2 * m[0] * dh; j.bu = 2 * m[1] * dv;
    j.av = 2 * m[2] * dh; j.bv = 2 * m[3] * dv;
    j.cu = (int64_t)m[0] * dh + (int64_t)m[1] * dv + 2 * (int64_t)m[4] - (int64_t)65536 * sh;
    j.cv = (int64_t)m[2] * dh + (int64_t)m[3] * dv + 2 * (int64_t)m[5] - (int64_t)65536 * sv;
    j.su = 8u + (uint32_t)sh; j.sv = 8u + (uint32_t)sv;
    j.border = (uint32_t)border; j.fill = fill;
    j.tiles_x = (mx + HVQ_WP_TW - 1u) / HVQ_WP_TW;
    j.tiles = j.tiles_x * ((my + HVQ_WP_TH - 1u) / HVQ_WP_TH);
    j.pad[0] = j.pad[1] = 0;
    hvq_wp_choose(&j, force);
    return j;
}

#endif
