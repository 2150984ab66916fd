/*
 * hvq_corner.h -- what the corner kernels (hvq_corner.hip), the runtime (hvq_corner_pictures) and the tests' fake device share: the job
 * record, the response arithmetic, and the phases of a tile, of the row counts, of the scan and of the list, written per lane: a kernel
 * calls a phase with its lane and puts a barrier behind it, the fake device calls it for every lane in turn.  C++ that compiles for the
 * host and the device alike: integers only, except the first guess of the one square root.  include/hvqm4_amd.h specifies the values.
 *
 * The ranges.  A Sobel gradient is at most 4 x 255 = 1020, a product at most 1020^2 < 2^20, a sum over (2r + 1)^2 <= 49 positions at
 * most 49 x 1020^2 = 50 979 600 < 2^26: A, C and |B| are 32-bit, T = A + C < 2^27.
 *   Harris   A C >= B^2 (Cauchy-Schwarz), so 0 <= 256 (A C - B^2) < 2^8 2^52 = 2^60, and 0 <= k T^2 <= 2^6 2^54 = 2^60: |R| < 2^60 < 2^61.
 *   Min-eig  (A - C)^2 < 2^52 and 4 B^2 < 2^54: the radicand is below 2^55, its root below 2^27.5 and at most T: 0 <= R < 2^27.
 *
 * A tile in LDS (HVQ_CR_LDS dwords; with h = nms + radius, the tile at (x0, y0)):
 *   S  the staged bytes: rows y0 - h - 1 .. y0 + 16 + h, columns x0 - 12 .. x0 + 75, every position clamped into the plane when staged.
 *   G  the gradients at rows y0 - h .., columns x0 - h ..: gx in the low half of a dword, gy in the high half.
 *   H  three planes: the sums of gx gx, gx gy, gy gy over the 2r + 1 columns around (row of G, column x0 - nms ..).
 *   R  the responses as qwords, rows y0 - nms .., columns x0 - nms ..; a position outside the plane holds HVQ_CR_NONE, which beats
 *      nothing.  R lies over S and G: a barrier stands between the last read of G and the first store of R.
 */
#ifndef HVQ_CORNER_H
#define HVQ_CORNER_H

#include <stdint.h>

#include "hvq_desc.h"

#define HVQ_CR_HARRIS    0u                                           /* HVQ_CRN_HARRIS, HVQ_CRN_MIN_EIGEN of include/hvqm4_amd.h */
#define HVQ_CR_MIN_EIGEN 1u
#define HVQ_CR_NONE      INT64_MIN

/* ------------------------------------------------------------------------------------------------ the job (host) */
/* `mask` is the mask picture, off[p] and dw[p] the byte offset and the dwords of its plane p */
static inline HvqCornerJob hvq_cr_job(uint64_t src, uint64_t mask, const uint64_t off[3], const uint32_t dw[3], uint32_t plane, uint64_t points,
                                      uint64_t rows, uint64_t response, uint32_t nx, uint32_t ny, uint32_t mode, uint32_t radius, uint32_t k,
                                      uint32_t nms, uint32_t margin, int64_t threshold, uint32_t cap)
{
    HvqCornerJob j;
    j.src = src; j.mask = mask + off[plane]; j.points = points; j.rows = rows; j.response = response;
    j.threshold = threshold;
    j.nx = nx; j.ny = ny;                                            /* nx is a multiple of 4 */
    j.tx = (nx + HVQ_CR_TX - 1u) / HVQ_CR_TX;
    j.ty = (ny + HVQ_CR_TY - 1u) / HVQ_CR_TY;
    j.mode = mode; j.radius = radius; j.k = k; j.nms = nms; j.margin = margin; j.cap = cap;
    for (uint32_t f = 0, p = 0; p < 3u; ++p) {
        if (p == plane) continue;
        j.fill[f] = mask + off[p];
        j.fill_dwords[f] = dw[p];
        j.fill_value[f] = p ? 0x80808080u : 0u;
        j.fill_tiles[f] = (dw[p] + HVQ_CR_FILL - 1u) / HVQ_CR_FILL;
        ++f;
    }
    return j;
}

static inline uint32_t hvq_cr_tiles(const HvqCornerJob &j) { return j.tx * j.ty + j.fill_tiles[0] + j.fill_tiles[1]; }

/* ------------------------------------------------------------------------------------------------ the lanes' code */
#if defined(HVQ_CR_PLAIN) || defined(__HIPCC__)

#if defined(HVQ_CR_PLAIN)
#define HVQ_CR_FN static inline
#else
#define HVQ_CR_FN __device__ static inline __attribute__((always_inline))
#endif

typedef struct __attribute__((aligned(16))) HvqCrPoint { int64_t v[4]; } HvqCrPoint;
typedef struct __attribute__((aligned(16))) HvqCrPair { int64_t v[2]; } HvqCrPair;

/* floor(sqrt(v)), v < 2^55: a double-precision guess, which is off by one at the most, set right by integer comparisons */
HVQ_CR_FN uint64_t hvq_cr_isqrt(uint64_t v)
{
    uint64_t s = (uint64_t)__builtin_sqrt((double)v);
    for (uint32_t i = 0; i < 4u && s * s > v; ++i) --s;
    for (uint32_t i = 0; i < 4u && (s + 1u) * (s + 1u) <= v; ++i) ++s;
    return s;
}

/* the response of the structure sums A = sum gx gx, B = sum gx gy, C = sum gy gy */
HVQ_CR_FN int64_t hvq_cr_response(uint32_t mode, uint32_t k, uint32_t A, int32_t B, uint32_t C)
{
    const uint64_t T = (uint64_t)A + C, bb = (uint64_t)((int64_t)B * B);
    if (mode == HVQ_CR_HARRIS) return (int64_t)(256u * ((uint64_t)A * C - bb)) - (int64_t)((uint64_t)k * T * T);
    const int64_t d = (int64_t)A - (int64_t)C;
    return (int64_t)(T - hvq_cr_isqrt((uint64_t)(d * d) + 4u * bb));
}

/* a sample of the plane, the position clamped into it */
HVQ_CR_FN int32_t hvq_cr_sample(const HvqCornerJob &J, int32_t y, int32_t x)
{
    const int32_t cy = y < 0 ? 0 : y >= (int32_t)J.ny ? (int32_t)J.ny - 1 : y, cx = x < 0 ? 0 : x >= (int32_t)J.nx ? (int32_t)J.nx - 1 : x;
    return ((const uint8_t *)(uintptr_t)J.src)[(uint32_t)cy * J.nx + (uint32_t)cx];
}

/* the response at (x, y) from the plane itself: what launch 4 stores for the few corners */
HVQ_CR_FN int64_t hvq_cr_response_at(const HvqCornerJob &J, uint32_t x, uint32_t y)
{
    const int32_t r = (int32_t)J.radius;
    uint32_t A = 0u, C = 0u;
    int32_t B = 0;
    for (int32_t py = (int32_t)y - r; py <= (int32_t)y + r; ++py)
        for (int32_t px = (int32_t)x - r; px <= (int32_t)x + r; ++px) {
            const int32_t a00 = hvq_cr_sample(J, py - 1, px - 1), a01 = hvq_cr_sample(J, py - 1, px), a02 = hvq_cr_sample(J, py - 1, px + 1);
            const int32_t a10 = hvq_cr_sample(J, py, px - 1), a12 = hvq_cr_sample(J, py, px + 1);
            const int32_t a20 = hvq_cr_sample(J, py + 1, px - 1), a21 = hvq_cr_sample(J, py + 1, px), a22 = hvq_cr_sample(J, py + 1, px + 1);
            const int32_t gx = a02 + 2 * a12 + a22 - a00 - 2 * a10 - a20, gy = a20 + 2 * a21 + a22 - a00 - 2 * a01 - a02;
            A += (uint32_t)(gx * gx); B += gx * gy; C += (uint32_t)(gy * gy);
        }
    return hvq_cr_response(J.mode, J.k, A, B, C);
}

/* ---- launch 1: a tile.  `tile` < tx ty; L is the workgroup's HVQ_CR_LDS dwords. */
HVQ_CR_FN void hvq_cr_tile_at(const HvqCornerJob &J, uint32_t tile, int32_t *x0, int32_t *y0)
{
    *x0 = (int32_t)((tile % J.tx) * HVQ_CR_TX);
    *y0 = (int32_t)((tile / J.tx) * HVQ_CR_TY);
}

/* S: the staged dwords, 16 + 2 (h + 1) rows of HVQ_CR_SD.  A dword of the row lies inside the plane or outside it as a whole (nx and
 * x0 - HVQ_CR_HX are multiples of 4); one outside repeats the row's first or last byte */
HVQ_CR_FN void hvq_cr_stage(const HvqCornerJob &J, uint32_t tile, uint32_t lane, uint32_t *L)
{
    int32_t x0, y0;
    hvq_cr_tile_at(J, tile, &x0, &y0);
    const uint32_t halo = J.nms + J.radius + 1u, n = (HVQ_CR_TY + 2u * halo) * HVQ_CR_SD;
    const uint32_t *src = (const uint32_t *)(uintptr_t)J.src;
    for (uint32_t i = lane; i < n; i += HVQ_CR_LANES) {
        const uint32_t sy = i / HVQ_CR_SD, sd = i % HVQ_CR_SD;
        int32_t y = y0 - (int32_t)halo + (int32_t)sy;
        y = y < 0 ? 0 : y >= (int32_t)J.ny ? (int32_t)J.ny - 1 : y;
        const int32_t x = x0 - (int32_t)HVQ_CR_HX + 4 * (int32_t)sd;
        const uint32_t row = (uint32_t)y * (J.nx >> 2);
        uint32_t v;
        if (x < 0) v = (src[row] & 255u) * 0x01010101u;
        else if (x >= (int32_t)J.nx) v = (src[row + (J.nx >> 2) - 1u] >> 24) * 0x01010101u;
        else v = src[row + ((uint32_t)x >> 2)];
        L[HVQ_CR_S_AT + i] = v;
    }
}

/* G: the gradients of 16 + 2 h rows and 64 + 2 h columns, once per position */
HVQ_CR_FN void hvq_cr_gradients(const HvqCornerJob &J, uint32_t lane, uint32_t *L)
{
    const uint32_t h = J.nms + J.radius, rows = HVQ_CR_TY + 2u * h, cols = HVQ_CR_TX + 2u * h, n = rows * cols;
    const uint8_t *S = (const uint8_t *)(L + HVQ_CR_S_AT);
    for (uint32_t i = lane; i < n; i += HVQ_CR_LANES) {
        const uint32_t gy = i / cols, gx = i % cols;
        /* the position in S: one row down (its halo is h + 1), HVQ_CR_HX - h columns to the right */
        const uint8_t *p = S + (gy + 1u) * (4u * HVQ_CR_SD) + gx + HVQ_CR_HX - h;
        const int32_t up = (int32_t)(4u * HVQ_CR_SD);
        const int32_t a00 = p[-up - 1], a01 = p[-up], a02 = p[-up + 1], a10 = p[-1], a12 = p[1], a20 = p[up - 1], a21 = p[up], a22 = p[up + 1];
        const int32_t dx = a02 + 2 * a12 + a22 - a00 - 2 * a10 - a20, dy = a20 + 2 * a21 + a22 - a00 - 2 * a01 - a02;
        L[HVQ_CR_G_AT + gy * HVQ_CR_GS + gx] = ((uint32_t)dx & 0xffffu) | ((uint32_t)dy << 16);
    }
}

HVQ_CR_FN void hvq_cr_products(uint32_t g, uint32_t *xx, int32_t *xy, uint32_t *yy)
{
    const int32_t dx = (int32_t)(int16_t)(g & 0xffffu), dy = (int32_t)g >> 16;
    *xx = (uint32_t)(dx * dx); *xy = dx * dy; *yy = (uint32_t)(dy * dy);
}

/* H: a lane slides along HVQ_CR_HSEG columns of one row of G: a product enters on the right and leaves on the left */
HVQ_CR_FN void hvq_cr_hsums(const HvqCornerJob &J, uint32_t lane, uint32_t *L)
{
    const uint32_t r = J.radius, rows = HVQ_CR_TY + 2u * (J.nms + r), cols = HVQ_CR_TX + 2u * J.nms;
    const uint32_t segs = (cols + HVQ_CR_HSEG - 1u) / HVQ_CR_HSEG;
    if (lane >= rows * segs) return;
    const uint32_t row = lane % rows, c0 = (lane / rows) * HVQ_CR_HSEG, c1 = c0 + HVQ_CR_HSEG < cols ? c0 + HVQ_CR_HSEG : cols;
    const uint32_t *G = L + HVQ_CR_G_AT + row * HVQ_CR_GS;
    uint32_t *H = L + HVQ_CR_H_AT + row * HVQ_CR_HS;
    uint32_t a = 0u, c = 0u, xx, yy;
    int32_t b = 0, xy;
    for (uint32_t t = 0; t < 2u * r; ++t) {                           /* column c of H sums the columns c .. c + 2 r of G */
        hvq_cr_products(G[c0 + t], &xx, &xy, &yy);
        a += xx; b += xy; c += yy;
    }
    for (uint32_t x = c0; x < c1; ++x) {
        hvq_cr_products(G[x + 2u * r], &xx, &xy, &yy);
        a += xx; b += xy; c += yy;
        H[x] = a; H[HVQ_CR_HPLANE + x] = (uint32_t)b; H[2u * HVQ_CR_HPLANE + x] = c;
        hvq_cr_products(G[x], &xx, &xy, &yy);
        a -= xx; b -= xy; c -= yy;
    }
}

/* R: a row of H enters below and leaves above; the response of a position outside the plane is HVQ_CR_NONE.  R lies over S and G: the
 * caller puts a barrier between hvq_cr_hsums and this */
HVQ_CR_FN void hvq_cr_responses(const HvqCornerJob &J, uint32_t tile, uint32_t lane, uint32_t *L)
{
    int32_t x0, y0;
    hvq_cr_tile_at(J, tile, &x0, &y0);
    const uint32_t r = J.radius, rows = HVQ_CR_TY + 2u * J.nms, cols = HVQ_CR_TX + 2u * J.nms;
    const uint32_t segs = (rows + HVQ_CR_VSEG - 1u) / HVQ_CR_VSEG;
    if (lane >= cols * segs) return;
    const uint32_t col = lane % cols, r0 = (lane / cols) * HVQ_CR_VSEG, r1 = r0 + HVQ_CR_VSEG < rows ? r0 + HVQ_CR_VSEG : rows;
    const uint32_t *H = L + HVQ_CR_H_AT + col;
    int64_t *R = (int64_t *)(L + HVQ_CR_R_AT);
    const int32_t x = x0 - (int32_t)J.nms + (int32_t)col;
    uint32_t a = 0u, c = 0u;
    int32_t b = 0;
    for (uint32_t t = 0; t < 2u * r; ++t) {                           /* row y of R sums the rows y .. y + 2 r of H */
        const uint32_t *h = H + (r0 + t) * HVQ_CR_HS;
        a += h[0]; b += (int32_t)h[HVQ_CR_HPLANE]; c += h[2u * HVQ_CR_HPLANE];
    }
    for (uint32_t ry = r0; ry < r1; ++ry) {
        const uint32_t *in = H + (ry + 2u * r) * HVQ_CR_HS, *out = H + ry * HVQ_CR_HS;
        a += in[0]; b += (int32_t)in[HVQ_CR_HPLANE]; c += in[2u * HVQ_CR_HPLANE];
        const int32_t y = y0 - (int32_t)J.nms + (int32_t)ry;
        const int inside = x >= 0 && x < (int32_t)J.nx && y >= 0 && y < (int32_t)J.ny;
        R[ry * HVQ_CR_HS + col] = inside ? hvq_cr_response(J.mode, J.k, a, b, c) : HVQ_CR_NONE;
        a -= out[0]; b -= (int32_t)out[HVQ_CR_HPLANE]; c -= out[2u * HVQ_CR_HPLANE];
    }
}

/* the lane's dword of the mask, and its four responses where they are asked for.  q beats p when R(q) > R(p), or R(q) == R(p) and q
 * comes first in raster order.  The order is total, so the rows may be looked at in any order: the nearest first, and a sample
 * leaves at the first row that beats it */
HVQ_CR_FN void hvq_cr_suppress(const HvqCornerJob &J, uint32_t tile, uint32_t lane, const uint32_t *L)
{
    int32_t x0, y0;
    hvq_cr_tile_at(J, tile, &x0, &y0);
    const uint32_t lx = (lane & 15u) * 4u, ly = lane >> 4, x = (uint32_t)x0 + lx, y = (uint32_t)y0 + ly, m = J.nms, g = J.margin;
    if (x >= J.nx || y >= J.ny) return;
    const int64_t *R = (const int64_t *)(L + HVQ_CR_R_AT);
    const int row_ok = y >= g && y + g < J.ny;
    uint32_t out = 0u;
    for (uint32_t s = 0; s < 4u; ++s) {
        const int64_t *p = R + (ly + m) * HVQ_CR_HS + lx + s + m;
        const int64_t v = *p;
        if (!row_ok || x + s < g || x + s + g >= J.nx || v < J.threshold) continue;
        uint32_t beaten = 0u;
        for (uint32_t t = 0; t <= 2u * m && !beaten; ++t) {          /* the rows 0, -1, 1, -2, 2, ...: what beats a sample is mostly next to it */
            const int32_t dy = (t & 1u) ? -(int32_t)((t + 1u) >> 1) : (int32_t)(t >> 1);
            const int64_t *q = p + dy * (int32_t)HVQ_CR_HS;
            for (int32_t dx = -(int32_t)m; dx <= (int32_t)m; ++dx) {
                const int64_t w = q[dx];
                beaten |= (w > v || (w == v && (dy < 0 || (dy == 0 && dx < 0)))) ? 1u : 0u;
            }
        }
        if (!beaten) out |= 255u << (8u * s);
    }
    ((uint32_t *)(uintptr_t)J.mask)[(y * J.nx + x) >> 2] = out;
    if (J.response) {
        HvqCrPair *to = (HvqCrPair *)((int64_t *)(uintptr_t)J.response + ((uint64_t)y * J.nx + x));
        const int64_t *p = R + (ly + m) * HVQ_CR_HS + lx + m;
        HvqCrPair a, b;
        a.v[0] = p[0]; a.v[1] = p[1]; b.v[0] = p[2]; b.v[1] = p[3];
        to[0] = a; to[1] = b;
    }
}

/* fill tile `t` of the plane f of the mask that is not analysed: sixteen bytes a lane (a plane is a multiple of 4 bytes, the last
 * dwords go one by one) */
HVQ_CR_FN void hvq_cr_fill(const HvqCornerJob &J, uint32_t f, uint32_t t, uint32_t lane)
{
    uint32_t *out = (uint32_t *)(uintptr_t)J.fill[f];
    const uint32_t d = t * HVQ_CR_FILL + lane * 4u, v = J.fill_value[f];
    for (uint32_t s = 0; s < 4u; ++s)
        if (d + s < J.fill_dwords[f]) out[d + s] = v;
}

/* ---- launches 2 and 4: dword d of row y of the mask, 0 beyond the row */
HVQ_CR_FN uint32_t hvq_cr_mask_dword(const HvqCornerJob &J, uint32_t y, uint32_t d)
{
    return d < (J.nx >> 2) ? ((const uint32_t *)(uintptr_t)J.mask)[y * (J.nx >> 2) + d] : 0u;
}
/* launch 2 leaves the row's count in rows[y]; launch 3 turns the counts into the index */
HVQ_CR_FN void hvq_cr_count_store(const HvqCornerJob &J, uint32_t y, uint32_t count) { ((uint32_t *)(uintptr_t)J.rows)[y] = count; }

/* ---- launch 3: ONE workgroup a picture.  Lane l owns the rows l per .. l per + per - 1, per = ceil(ny / HVQ_CR_LANES) */
HVQ_CR_FN uint32_t hvq_cr_scan_sum(const HvqCornerJob &J, uint32_t lane)
{
    const uint32_t *rows = (const uint32_t *)(uintptr_t)J.rows;
    const uint32_t per = (J.ny + HVQ_CR_LANES - 1u) / HVQ_CR_LANES;
    uint32_t sum = 0u;
    for (uint32_t y = lane * per; y < lane * per + per && y < J.ny; ++y) sum += rows[y];
    return sum;
}
/* `before`: the corners of the lanes before this one */
HVQ_CR_FN void hvq_cr_scan_store(const HvqCornerJob &J, uint32_t lane, uint32_t before)
{
    uint32_t *rows = (uint32_t *)(uintptr_t)J.rows;
    const uint32_t per = (J.ny + HVQ_CR_LANES - 1u) / HVQ_CR_LANES;
    for (uint32_t y = lane * per; y < lane * per + per && y < J.ny; ++y) {
        const uint32_t c = rows[y];
        rows[y] = before;
        before += c;
    }
}
HVQ_CR_FN void hvq_cr_head(const HvqCornerJob &J, uint32_t K)
{
    ((uint32_t *)(uintptr_t)J.rows)[J.ny] = K;
    HvqCrPoint h;
    h.v[0] = K; h.v[1] = K < J.cap ? K : J.cap; h.v[2] = 0; h.v[3] = 0;
    *(HvqCrPoint *)(uintptr_t)J.points = h;
}

/* ---- launch 4: corner number j (from 1) of the picture, at (x, y) */
HVQ_CR_FN void hvq_cr_emit(const HvqCornerJob &J, uint32_t x, uint32_t y, uint32_t j)
{
    if (j > J.cap) return;
    HvqCrPoint p;
    p.v[0] = x; p.v[1] = y; p.v[2] = hvq_cr_response_at(J, x, y); p.v[3] = (int64_t)y * J.nx + x;
    ((HvqCrPoint *)(uintptr_t)J.points)[j] = p;
}

#endif
#endif
