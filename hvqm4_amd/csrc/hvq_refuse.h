/*
 * hvq_refuse.h -- what a parsed picture READS, checked on the finished blob: one rule, compiled into the host parser
 * (hvq_parse.c) and into the GPU parser (hvq_gparse_core.h, all its paths), so that the two cannot disagree.
 *
 * The reference reads where the stream points (refuse, never decode differently):
 *   - every picture is its own allocation of pic_bytes (h4m:2347-2349).  A motion-compensated block (h4m:1242-1294, 1327-1355,
 *     1862-1910) or a sample of a USED window basis (h4m:734-773) outside [0, pic_bytes) of the referenced picture is foreign
 *     memory.  Reads that leave their plane but stay inside the buffer (luma into U, U into V, chroma backwards) are defined and
 *     are decoded as the reference decodes them.
 *   - a section of size 0 is a NULL buffer (h4m:1061-1071): anything read from it, and any symbol of a prefix tree whose carrier
 *     section is empty, is a NULL dereference resp. a leaf left by an earlier picture.
 * Either raises HVQ_F_CLAMPED.  Which sections a picture reads follows from its block types alone -- the loops of the reference
 * are driven by them (h4m:1073-1130, 1670-1740, 1789-1827, 1862-1955) -- except the DC run lengths of an I picture (a zero delta is not
 * visible in the values): those sections are reported by the parsers' DC loops (HVQ_SEC_RLE in `read_mask`).
 *
 * The walk is per run of 64 blocks (wave_base[] gives the run's first payload dword, the type bytes the payload lengths), a
 * minimum and a maximum per block and per basis: nothing per sample.
 */
#ifndef HVQ_REFUSE_H
#define HVQ_REFUSE_H

#include "hvq_desc.h"

#ifndef GP_G
#define HVQ_REFUSE_OWN_GP_G
#define GP_G
#endif

/* section numbers of the offset tables (h4m:1979-1993, 2030-2044) */
#define HVQ_SEC_BN(x)   (2 * (x))          /* block kinds: luma, chroma */
#define HVQ_SEC_BNR(x)  (2 * (x) + 1)      /* their zero runs */
#define HVQ_SEC_DC(p)   (4 + 3 * (p))
#define HVQ_SEC_BT(p)   (5 + 3 * (p))
#define HVQ_SEC_FX(p)   (6 + 3 * (p))
#define HVQ_SEC_RLE(p)  (13 + (p))         /* I pictures */
#define HVQ_SEC_MVH     13                 /* P/B pictures */
#define HVQ_SEC_MVV     14
#define HVQ_SEC_MTYPE   15
#define HVQ_SEC_MPROC   16
#define HVQ_SEC_OUTSIDE 0x80000000u        /* in the mask of empty sections: some section's 4-byte size does not lie inside the picture --
                                              the reference reads it wherever the offset table points, used or not (h4m:1061-1071) */

typedef struct HvqReadsGeom {
    const GP_G uint8_t *blob;
    uint32_t map_off[3], run_first[3], plane_off[3];
    int hb[3], vb[3];
    uint32_t mv_off, wave_base_off, pool_off, pool_dwords, pic_bytes, total_runs;
    int w, wshift, hshift, is15, landscape, mcb_w, is_pb;
} HvqReadsGeom;

/* the sections whose tree is carried by another one (h4m:1996-1999, 2045-2050): reading them reads that tree */
HVQ_HD static inline uint32_t hvq_reads_close(uint32_t need, int is_pb)
{
    if (need & (1u << HVQ_SEC_BN(1))) need |= 1u << HVQ_SEC_BN(0);
    if (need & ((1u << HVQ_SEC_BNR(1)) | (is_pb ? 0u : (7u << HVQ_SEC_RLE(0))))) need |= 1u << HVQ_SEC_BNR(0);
    if (need & ((1u << HVQ_SEC_DC(1)) | (1u << HVQ_SEC_DC(2)))) need |= 1u << HVQ_SEC_DC(0);
    if (need & ((1u << HVQ_SEC_BT(1)) | (1u << HVQ_SEC_BT(2)))) need |= 1u << HVQ_SEC_BT(0);
    if (is_pb) {
        if (need & (1u << HVQ_SEC_MVV)) need |= 1u << HVQ_SEC_MVH;
        if (need & (1u << HVQ_SEC_MPROC)) need |= 1u << HVQ_SEC_MTYPE;
    }
    return need;
}

/* runs first, first + step, ... of the picture: bit 31 = a read outside the referenced picture, bits 0-16 = the sections read */
#define HVQ_READS_OUTSIDE 0x80000000u
HVQ_HD static inline uint32_t hvq_reads_walk(const HvqReadsGeom *g, uint32_t first, uint32_t step)
{
    const GP_G uint32_t *wave_base = (const GP_G uint32_t *)(g->blob + g->wave_base_off);
    const GP_G uint32_t *pool = (const GP_G uint32_t *)(g->blob + g->pool_off);
    const GP_G int16_t *mvs = (const GP_G int16_t *)(g->blob + g->mv_off);
    uint32_t out = 0;
    for (uint32_t r = first; r < g->total_runs; r += step) {
        const int i = r >= g->run_first[2] ? 2 : (r >= g->run_first[1] ? 1 : 0);
        const int ws = i ? g->wshift : 0, hs = i ? g->hshift : 0, pw = g->w >> ws;
        const int hb = g->hb[i], stride = hb + 2;
        const uint32_t nblocks = (uint32_t)hb * (uint32_t)g->vb[i];
        const uint32_t b0 = (r - g->run_first[i]) * 64u, b1 = b0 + 64u < nblocks ? b0 + 64u : nblocks;
        const GP_G uint8_t *map = g->blob + g->map_off[i];
        uint32_t off = b0 < nblocks ? wave_base[r] : 0u;
        int by = (int)(b0 / (uint32_t)hb), bx = (int)(b0 - (uint32_t)by * (uint32_t)hb);
        for (uint32_t b = b0; b < b1; ++b) {
            const uint32_t e = (uint32_t)(by + 1) * (uint32_t)stride + (uint32_t)(bx + 1);
            const uint32_t type = map[2u * e + 1u];
            const uint32_t kind = (g->is_pb || i) ? (type & 0xFu) : type;
            const uint32_t n = hvq_payload_dwords(type, g->is_pb, !g->is_pb && i == 0);
            if (off + n > g->pool_dwords) break;                    /* a refused picture whose pool was never laid out */
            if (!g->is_pb) {
                out |= (1u << HVQ_SEC_BN(i ? 1 : 0)) | (1u << HVQ_SEC_DC(i));
                if (i == 0 && type == 0) out |= 1u << HVQ_SEC_BNR(0);
                if (i == 1 && type == 0 && g->blob[g->map_off[2] + 2u * e + 1u] == 0) out |= 1u << HVQ_SEC_BNR(1);
                if (kind == 6) out |= 1u << HVQ_SEC_FX(i);
                else if (n) out |= (1u << HVQ_SEC_FX(i)) | (1u << HVQ_SEC_BT(i));
            } else if (!(type & 0x60u)) {                           /* intra macroblock: h4m:1649-1668, 1789-1827 */
                out |= (1u << HVQ_SEC_BN(0)) | (1u << HVQ_SEC_BN(1)) | (1u << HVQ_SEC_DC(i)) | (1u << HVQ_SEC_MTYPE);
                if (i == 0 && kind == 0) out |= 1u << HVQ_SEC_BNR(0);
                if (i == 1 && kind == 0 && (g->blob[g->map_off[2] + 2u * e + 1u] & 0xFu) == 0) out |= 1u << HVQ_SEC_BNR(1);
                if (kind == 6) out |= 1u << HVQ_SEC_FX(i);
                else if (n) out |= (1u << HVQ_SEC_FX(i)) | (1u << HVQ_SEC_BT(i));
            } else {
                const int proc = (type & 0x10u) != 0;
                out |= (1u << HVQ_SEC_MTYPE) | (1u << HVQ_SEC_MPROC) | (1u << HVQ_SEC_MVH) | (1u << HVQ_SEC_MVV);
                if (!proc) {                                        /* its block kinds are coded: h4m:1692-1740 */
                    out |= (1u << HVQ_SEC_BN(0)) | (1u << HVQ_SEC_BN(1));
                    if (i == 0 && kind == 0) out |= 1u << HVQ_SEC_BNR(0);
                    if (i == 1 && kind == 0 && (g->blob[g->map_off[2] + 2u * e + 1u] & 0xFu) == 0) out |= 1u << HVQ_SEC_BNR(1);
                }
                if (!proc && kind == 6) out |= 1u << HVQ_SEC_FX(i);
                else {
                    /* the macroblock's target (h4m:1954-1955) and the block's reads: first sample .. last sample of the last row,
                     * one more row / column at a half-sample position (h4m:1242-1294) */
                    const int mx = bx >> (1 - ws), my = by >> (1 - hs);
                    const int rx = mvs[2 * (my * g->mcb_w + mx)], ry = mvs[2 * (my * g->mcb_w + mx) + 1];
                    const int pdx = rx >> ws, pdy = ry >> hs;
                    const int hx = g->is15 ? (pdx & 1) : (rx & 1), hy = g->is15 ? (pdy & 1) : (ry & 1);
                    const int dx = bx & ((2 >> ws) - 1), dy = by & ((2 >> hs) - 1);   /* the block inside its macroblock */
                    const int32_t lo = (int32_t)g->plane_off[i] + ((pdy >> 1) + dy * 4) * pw + (pdx >> 1) + dx * 4;
                    const int32_t hi = lo + (3 + hy) * pw + 3 + hx;
                    if (lo < 0 || hi >= (int32_t)g->pic_bytes) out |= HVQ_READS_OUTSIDE;
                    if (!proc && kind) {                            /* MC residual: two scalars, kind - 1 window bases (h4m:1379-1420) */
                        out |= 1u << HVQ_SEC_DC(i);
                        if (kind > 1) out |= (1u << HVQ_SEC_FX(i)) | (1u << HVQ_SEC_BT(i));
                        const int32_t win = g->landscape ? rx / 2 + (ry / 2 - 16) * g->w - 32 : rx / 2 + (ry / 2 - 32) * g->w - 16;
                        for (uint32_t k = 0; k + 1 < kind; ++k) {   /* h4m:734-773 */
                            const uint32_t word = pool[off + 2u + k];
                            const int off_long = (int)(word & 0x3Fu), off_short = (int)((word >> 6) & 0x1Fu);
                            const int s_long = (int)((word >> 11) & 1u), s_short = (int)((word >> 12) & 1u);
                            const int32_t q = win + (g->landscape ? g->w * off_short + off_long : g->w * off_long + off_short);
                            const int32_t xs = 1 << (g->landscape ? s_long : s_short), ys = g->w << (g->landscape ? s_short : s_long);
                            if (q < 0 || q + 3 * ys + 3 * xs >= (int32_t)g->pic_bytes) out |= HVQ_READS_OUTSIDE;
                        }
                    }
                }
            }
            off += n;
            if (++bx == hb) { bx = 0; ++by; }
        }
    }
    return out;
}

/* the verdict from everything the walk (and, I pictures, the DC loops) found: `dead` = sections of size 0 */
HVQ_HD static inline uint32_t hvq_reads_flags(uint32_t found, uint32_t dead, int is_pb)
{
    const uint32_t need = hvq_reads_close(found & 0x1FFFFu, is_pb);
    return ((found & HVQ_READS_OUTSIDE) || (need & dead) || (dead & HVQ_SEC_OUTSIDE)) ? HVQ_F_CLAMPED : 0u;
}

#ifdef HVQ_REFUSE_OWN_GP_G
#undef GP_G
#undef HVQ_REFUSE_OWN_GP_G
#endif
#endif
