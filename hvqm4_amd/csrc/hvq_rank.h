/*
 * hvq_rank.h -- what the rank kernel (hvq_rank.hip), the runtime (hvq_rank_pictures) and the tests' fake device share: the choice of a
 * plane's body and its job record, the index arithmetic of a tile (which source row and dword a staged dword is, the edge sample in the
 * halo), the packed min / max of four samples a dword, and the phases of the bodies themselves, written per lane over the tile's LDS
 * arrays: the kernel calls a phase with its lane and puts a barrier behind it, the fake device calls it for every lane in turn.  Plain
 * C++ that compiles for the host and the device alike.  include/hvqm4_amd.h specifies the values.
 *
 * The staged tile.  rows = HVQ_RK_TH + 2 r staged rows (r: ry of the min/max body, 1 or 2 of the medians), staged row rr = source row
 * r0 + rr - r clamped into the plane; each HVQ_RK_ROW_DWORDS aligned dwords, the source bytes c0 - 16 .. c0 + 79.  A dword that lies
 * outside the row holds the row's edge sample four times: rows AND columns are clamped when staging, so that no later phase clamps
 * anything and every window of a target, as the header counts it, lies in the staged bytes as it is.
 *
 * Four samples a dword.  There is no 8-bit min / max: the even bytes (v & 0x00ff00ff) and the odd ones (v & 0xff00ff00, left where they
 * are: a byte in the upper half of a 16-bit lane orders like the byte) go through the packed 16-bit min / max.  hvq_rk_min4 / max4 need
 * five operations a dword: the upper byte of the 16-bit min of the unmasked halves IS the min of the upper bytes.  The medians keep a
 * dword unpacked as a pair through their networks: two operations a min or max.
 */
#ifndef HVQ_RANK_H
#define HVQ_RANK_H

#include <stdint.h>

#include "hvq_desc.h"

#if defined(__HIPCC__)
#define HVQ_RK_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define HVQ_RK_FN static inline
#endif

/* the operations of include/hvqm4_amd.h (HVQ_RNK_*) */
#define HVQ_RK_OP_MIN    0u
#define HVQ_RK_OP_MAX    1u
#define HVQ_RK_OP_RANGE  2u
#define HVQ_RK_OP_MEDIAN 3u

/* ------------------------------------------------------------------------------------------------ the job of a plane (host) */
/* the body of a plane: the copy body for what copies the plane (radius 0 under MIN, MAX and MEDIAN) unless `general` switches it off
 * (hvq_rank_force_general); a median of radius 0 then runs the min/max body as MIN of radius 0 */
static inline HvqRankJob hvq_rk_job(uint64_t src, uint64_t dst, uint32_t nx, uint32_t ny, uint32_t op, uint32_t rx, uint32_t ry, int general)
{
    HvqRankJob j;
    j.src = src; j.dst = dst; j.nx = nx; j.ny = ny; j.op = op; j.rx = rx; j.ry = ry;
    if (op == HVQ_RK_OP_MEDIAN && rx) j.body = rx == 1u ? HVQ_RK_MED3 : HVQ_RK_MED5;
    else if (op != HVQ_RK_OP_RANGE && !rx && !ry && !general) j.body = HVQ_RK_COPY;
    else j.body = HVQ_RK_MINMAX;
    if (j.body == HVQ_RK_MINMAX && op == HVQ_RK_OP_MEDIAN) j.op = HVQ_RK_OP_MIN;
    const uint32_t tw = j.body == HVQ_RK_COPY ? HVQ_RK_CTW : HVQ_RK_TW, th = j.body == HVQ_RK_COPY ? HVQ_RK_CTH : HVQ_RK_TH;
    j.tiles_x = (nx + tw - 1u) / tw;
    j.tiles = j.tiles_x * ((ny + th - 1u) / th);
    return j;
}

/* ------------------------------------------------------------------------------------------------ staging */
HVQ_RK_FN uint32_t hvq_rk_stage_row(uint32_t r0, uint32_t rr, uint32_t r, uint32_t ny)
{
    const int32_t y = (int32_t)(r0 + rr) - (int32_t)r;
    return y < 0 ? 0u : y >= (int32_t)ny ? ny - 1u : (uint32_t)y;
}
/* dword k of a staged row is the row's dword c0 / 4 - 4 + k; one outside the row is loaded from the nearest inside ... */
HVQ_RK_FN uint32_t hvq_rk_stage_dword(uint32_t c0, uint32_t k, uint32_t nx)
{
    const int32_t d = (int32_t)(c0 >> 2) - (int32_t)(HVQ_RK_HALO >> 2) + (int32_t)k, last = (int32_t)(nx >> 2) - 1;
    return d < 0 ? 0u : d > last ? (uint32_t)last : (uint32_t)d;
}
/* ... and becomes the edge sample four times: the first byte of the row left of it, the last byte right of it (nx is a multiple of 4: a
 * dword lies inside the row or outside) */
HVQ_RK_FN uint32_t hvq_rk_stage_value(uint32_t v, uint32_t c0, uint32_t k, uint32_t nx)
{
    const int32_t d = (int32_t)(c0 >> 2) - (int32_t)(HVQ_RK_HALO >> 2) + (int32_t)k, last = (int32_t)(nx >> 2) - 1;
    return d < 0 ? (v & 0xffu) * 0x01010101u : d > last ? (v >> 24) * 0x01010101u : v;
}

/* ------------------------------------------------------------------------------------------------ four samples a dword */
HVQ_RK_FN uint32_t hvq_rk_pkmin(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short hvq_rk_us2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(hvq_rk_us2, a), __builtin_bit_cast(hvq_rk_us2, b)));
#else
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al < bl ? al : bl) | (ah < bh ? ah : bh) << 16;
#endif
}
HVQ_RK_FN uint32_t hvq_rk_pkmax(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short hvq_rk_us2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(hvq_rk_us2, a), __builtin_bit_cast(hvq_rk_us2, b)));
#else
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al : bl) | (ah > bh ? ah : bh) << 16;
#endif
}
#define HVQ_RK_EVEN 0x00ff00ffu
#define HVQ_RK_ODD  0xff00ff00u
HVQ_RK_FN uint32_t hvq_rk_min4(uint32_t a, uint32_t b) { return (hvq_rk_pkmin(a, b) & HVQ_RK_ODD) | hvq_rk_pkmin(a & HVQ_RK_EVEN, b & HVQ_RK_EVEN); }
HVQ_RK_FN uint32_t hvq_rk_max4(uint32_t a, uint32_t b) { return (hvq_rk_pkmax(a, b) & HVQ_RK_ODD) | hvq_rk_pkmax(a & HVQ_RK_EVEN, b & HVQ_RK_EVEN); }

/* bytes sh .. sh + 3 of the eight bytes lo, hi (sh 0 .. 3): v_alignbyte_b32 */
HVQ_RK_FN uint32_t hvq_rk_align(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (sh & 3u)));
#endif
}
/* the four bytes from byte `at` of an array of aligned dwords: the dword it starts in and the one behind */
HVQ_RK_FN uint32_t hvq_rk_read(const uint32_t *row, uint32_t at) { return hvq_rk_align(row[(at >> 2) + 1u], row[at >> 2], at & 3u); }

/* a dword unpacked for the medians' networks */
typedef struct HvqRkPair { uint32_t e, o; } HvqRkPair;
HVQ_RK_FN HvqRkPair hvq_rk_unpack(uint32_t v) { HvqRkPair p; p.e = v & HVQ_RK_EVEN; p.o = v & HVQ_RK_ODD; return p; }
HVQ_RK_FN uint32_t hvq_rk_pack(HvqRkPair p) { return p.e | p.o; }
HVQ_RK_FN HvqRkPair hvq_rk_pmin(HvqRkPair a, HvqRkPair b) { HvqRkPair p; p.e = hvq_rk_pkmin(a.e, b.e); p.o = hvq_rk_pkmin(a.o, b.o); return p; }
HVQ_RK_FN HvqRkPair hvq_rk_pmax(HvqRkPair a, HvqRkPair b) { HvqRkPair p; p.e = hvq_rk_pkmax(a.e, b.e); p.o = hvq_rk_pkmax(a.o, b.o); return p; }

/* ------------------------------------------------------------------------------------------------ the min/max body
 * A window of w = 2 r + 1 is built by doubling: m_1 = a, m_2c[x] = min(m_c[x], m_c[x + c]) while 2 c < w, and one last step
 * min(m_c[x], m_c[x + w - c]) of two windows that overlap: ceil(log2 w) steps, five at radius 15, whatever the radius in between.
 * Horizontal first, over whole staged rows; its last step moves to the tile's 16 dwords a row and to the window's centre.  Then the same
 * down the rows; the last step leaves a lane's dword in a register.  RANGE carries min and max through the same steps, each in its own
 * pair of arrays; both start from the staged rows.  A step reads one array and writes another: a barrier between two steps. */
#define HVQ_RK_STEPS(w, c) for (c = 1u; (w) - c > c; c <<= 1)      /* the doubling steps; behind it the last step's offset is w - c */

/* a doubling step over the staged rows: dword idx = rr * 24 + k with the bytes s further right (the dwords past the row's end are
 * replaced by its last: what they feed is never looked at) */
HVQ_RK_FN void hvq_rk_h_step(uint32_t lane, uint32_t rows, uint32_t s, int do_min, int do_max, const uint32_t *smin, uint32_t *dmin, const uint32_t *smax, uint32_t *dmax)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < 5u; ++u) {
        const uint32_t idx = lane + HVQ_RK_LANES * u;
        if (idx >= rows * HVQ_RK_ROW_DWORDS) continue;
        const uint32_t rr = idx / HVQ_RK_ROW_DWORDS, k = idx - rr * HVQ_RK_ROW_DWORDS, kb = k + (s >> 2);
        const uint32_t i0 = rr * HVQ_RK_ROW_DWORDS + (kb < HVQ_RK_ROW_DWORDS - 1u ? kb : HVQ_RK_ROW_DWORDS - 1u);
        const uint32_t i1 = rr * HVQ_RK_ROW_DWORDS + (kb + 1u < HVQ_RK_ROW_DWORDS - 1u ? kb + 1u : HVQ_RK_ROW_DWORDS - 1u);
        if (do_min) dmin[idx] = hvq_rk_min4(smin[idx], hvq_rk_align(smin[i1], smin[i0], s & 3u));
        if (do_max) dmax[idx] = hvq_rk_max4(smax[idx], hvq_rk_align(smax[i1], smax[i0], s & 3u));
    }
}
/* the last horizontal step: target dword d of staged row rr (idx = rr * 16 + d) from the bytes 16 + 4 d - rx and s further right */
HVQ_RK_FN void hvq_rk_h_last(uint32_t lane, uint32_t rows, uint32_t rx, uint32_t s, int do_min, int do_max, const uint32_t *smin, uint32_t *dmin, const uint32_t *smax, uint32_t *dmax)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < 3u; ++u) {
        const uint32_t idx = lane + HVQ_RK_LANES * u;
        if (idx >= rows * 16u) continue;
        const uint32_t row = (idx >> 4) * HVQ_RK_ROW_DWORDS, at = HVQ_RK_HALO + 4u * (idx & 15u) - rx;
        if (do_min) dmin[idx] = hvq_rk_min4(hvq_rk_read(smin + row, at), hvq_rk_read(smin + row, at + s));
        if (do_max) dmax[idx] = hvq_rk_max4(hvq_rk_read(smax + row, at), hvq_rk_read(smax + row, at + s));
    }
}
/* a doubling step down the rows of the tile-wide arrays (a row past the last is replaced by the last) */
HVQ_RK_FN void hvq_rk_v_step(uint32_t lane, uint32_t rows, uint32_t s, int do_min, int do_max, const uint32_t *smin, uint32_t *dmin, const uint32_t *smax, uint32_t *dmax)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < 3u; ++u) {
        const uint32_t idx = lane + HVQ_RK_LANES * u;
        if (idx >= rows * 16u) continue;
        const uint32_t r2 = (idx >> 4) + s < rows - 1u ? (idx >> 4) + s : rows - 1u, other = r2 * 16u + (idx & 15u);
        if (do_min) dmin[idx] = hvq_rk_min4(smin[idx], smin[other]);
        if (do_max) dmax[idx] = hvq_rk_max4(smax[idx], smax[other]);
    }
}
/* the last vertical step: the lane's dword of the tile, dword lane & 15 of target row lane >> 4, from the rows lane >> 4 and s below */
HVQ_RK_FN uint32_t hvq_rk_v_last(uint32_t lane, uint32_t s, uint32_t op, const uint32_t *smin, const uint32_t *smax)
{
    const uint32_t other = lane + s * 16u;
    const uint32_t lo = op != HVQ_RK_OP_MAX ? hvq_rk_min4(smin[lane], smin[other]) : 0u;
    const uint32_t hi = op != HVQ_RK_OP_MIN ? hvq_rk_max4(smax[lane], smax[other]) : 0u;
    return op == HVQ_RK_OP_MIN ? lo : op == HVQ_RK_OP_MAX ? hi : hi - lo;      /* max >= min byte by byte: no borrow crosses a byte */
}

/* ------------------------------------------------------------------------------------------------ the median bodies
 * (1) The columns are sorted once for all the targets that share them: for tile row j and staged dword k (idx = j * 24 + k) the 3 or 5
 * samples under one another, four columns a dword, into one array per level, S[level * HVQ_RK_SORTED + idx].  (2) A lane reads the 3 or 5
 * neighbouring columns of its four targets from every level and selects. */
#define HVQ_RK_X(a, b) { const HvqRkPair lo_ = hvq_rk_pmin(v[a], v[b]), hi_ = hvq_rk_pmax(v[a], v[b]); v[a] = lo_; v[b] = hi_; }
#define HVQ_RK_LO(a, b) { v[a] = hvq_rk_pmin(v[a], v[b]); }
#define HVQ_RK_HI(a, b) { v[b] = hvq_rk_pmax(v[a], v[b]); }

HVQ_RK_FN void hvq_rk_med_sort3(uint32_t lane, const uint32_t *raw, uint32_t *S)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < 2u; ++u) {
        const uint32_t idx = lane + HVQ_RK_LANES * u;
        if (idx >= HVQ_RK_SORTED) continue;
        HvqRkPair v[3];
        for (uint32_t i = 0; i < 3u; ++i) v[i] = hvq_rk_unpack(raw[idx + HVQ_RK_ROW_DWORDS * i]);
        HVQ_RK_X(0, 1) HVQ_RK_X(1, 2) HVQ_RK_X(0, 1)
        for (uint32_t i = 0; i < 3u; ++i) S[HVQ_RK_SORTED * i + idx] = hvq_rk_pack(v[i]);
    }
}
HVQ_RK_FN void hvq_rk_med_sort5(uint32_t lane, const uint32_t *raw, uint32_t *S)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t u = 0; u < 2u; ++u) {
        const uint32_t idx = lane + HVQ_RK_LANES * u;
        if (idx >= HVQ_RK_SORTED) continue;
        HvqRkPair v[5];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < 5u; ++i) v[i] = hvq_rk_unpack(raw[idx + HVQ_RK_ROW_DWORDS * i]);
        HVQ_RK_X(0, 1) HVQ_RK_X(3, 4) HVQ_RK_X(2, 4) HVQ_RK_X(2, 3) HVQ_RK_X(0, 3) HVQ_RK_X(0, 2) HVQ_RK_X(1, 4) HVQ_RK_X(1, 3) HVQ_RK_X(1, 2)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < 5u; ++i) S[HVQ_RK_SORTED * i + idx] = hvq_rk_pack(v[i]);
    }
}
/* 3 x 3: the median of nine is the median of the largest of the columns' minima, the median of their medians and the smallest of their
 * maxima */
HVQ_RK_FN HvqRkPair hvq_rk_med3(HvqRkPair a, HvqRkPair b, HvqRkPair c) { return hvq_rk_pmax(hvq_rk_pmin(a, b), hvq_rk_pmin(hvq_rk_pmax(a, b), c)); }
HVQ_RK_FN uint32_t hvq_rk_med_select3(uint32_t lane, const uint32_t *S)
{
    HvqRkPair m[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 3u; ++i) {
        const uint32_t *p = S + HVQ_RK_SORTED * i + (lane >> 4) * HVQ_RK_ROW_DWORDS + (lane & 15u) + (HVQ_RK_HALO >> 2);
        const uint32_t x0 = p[-1], x1 = p[0], x2 = p[1];
        const HvqRkPair l = hvq_rk_unpack(hvq_rk_align(x1, x0, 3u)), c = hvq_rk_unpack(x1), r = hvq_rk_unpack(hvq_rk_align(x2, x1, 1u));
        m[i] = i == 0u ? hvq_rk_pmax(hvq_rk_pmax(l, c), r) : i == 1u ? hvq_rk_med3(l, c, r) : hvq_rk_pmin(hvq_rk_pmin(l, c), r);
    }
    return hvq_rk_pack(hvq_rk_med3(m[0], m[1], m[2]));
}
/* 5 x 5: v[5 column + level], every column sorted; a sorting network of 25 (the levels sorted across the columns, then an odd-even merge
 * sort over the anti-diagonals) from which every exchange that cannot swap on sorted columns and every half that the median does not
 * depend on is taken out (tools/median_network.py): 79 exchanges, 134 min / max; checked on all 6^5 0 / 1 patterns of sorted columns.  The
 * median leaves on 12. */
HVQ_RK_FN uint32_t hvq_rk_med_select5(uint32_t lane, const uint32_t *S)
{
    HvqRkPair v[25];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 5u; ++i) {
        const uint32_t *p = S + HVQ_RK_SORTED * i + (lane >> 4) * HVQ_RK_ROW_DWORDS + (lane & 15u) + (HVQ_RK_HALO >> 2);
        const uint32_t x0 = p[-1], x1 = p[0], x2 = p[1];
        v[i] = hvq_rk_unpack(hvq_rk_align(x1, x0, 2u));
        v[5u + i] = hvq_rk_unpack(hvq_rk_align(x1, x0, 3u));
        v[10u + i] = hvq_rk_unpack(x1);
        v[15u + i] = hvq_rk_unpack(hvq_rk_align(x2, x1, 1u));
        v[20u + i] = hvq_rk_unpack(hvq_rk_align(x2, x1, 2u));
    }
#define X HVQ_RK_X
#define LO HVQ_RK_LO
#define HI HVQ_RK_HI
    X(0,5) X(15,20) X(10,20) X(10,15) X(0,15) HI(0,10) X(5,20) X(5,15) X(5,10) X(1,6) X(16,21) X(11,21) X(11,16) X(1,16) HI(1,11)
    X(6,21) X(6,16) X(6,11) X(2,7) X(17,22) X(12,22) X(12,17) X(2,17) X(2,12) LO(7,22) X(7,17) X(7,12) X(3,8) X(18,23) X(13,23)
    X(13,18) X(3,18) X(3,13) LO(8,23) LO(8,18) X(8,13) X(4,9) X(19,24) X(14,24) X(14,19) X(4,19) X(4,14) LO(9,24) LO(9,19) X(9,14)
    HI(5,2) X(6,10) X(3,7) HI(6,3) X(10,7) X(10,3) HI(2,10) X(11,15) X(4,8) HI(11,4) X(15,8) X(15,4) X(12,16) X(20,9) X(12,20)
    LO(16,9) X(16,20) LO(4,20) X(4,12) LO(8,16) X(15,4) X(8,12) HI(3,4) HI(10,15) X(7,8) HI(7,15) HI(15,4) X(8,12) LO(13,17)
    LO(21,14) LO(13,21) LO(12,13) HI(4,12) HI(8,12)
#undef X
#undef LO
#undef HI
    return hvq_rk_pack(v[12]);
}

#endif
