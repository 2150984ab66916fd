/*
 * oracle/hvq_desc_recon.h -- TEST INFRASTRUCTURE ONLY: the view the scalar descriptor interpreter (hvq_desc_recon.c)
 * works on, and its entry points.  A front end fills the view -- from a blob header (hvqd_recon) or from an HvqJob record
 * (tests/native/fake_kernels.cpp) -- and says which tiles to reconstruct.
 */
#ifndef HVQ_DESC_RECON_H
#define HVQ_DESC_RECON_H

#include <stdint.h>

#include "hvq_desc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct HvqdPlane {
    const uint8_t *map;            /* entry [-1][-1] of the bordered map */
    uint8_t *dst;                  /* the plane inside the destination picture (a self-referencing P picture: inside its side buffer) */
    uint32_t plane_off;            /* byte offset of the plane inside a picture buffer (reference reads) */
    uint32_t tile_first;           /* first tile index of the plane */
    int hb, vb;                    /* 4x4 blocks per row, rows */
    int pw, ws, hs;                /* samples per row, subsampling shifts relative to luma */
} HvqdPlane;

typedef struct HvqdView {
    HvqdPlane pl[3];
    const uint32_t *pool;
    const uint32_t *wave_base;
    const int16_t *mvs;            /* NULL in I pictures */
    const uint8_t *ref0, *ref1;    /* "past" (macroblock type 1) and "future" (type 2) pictures */
    uint32_t slot_bytes;           /* readable bytes of a reference picture */
    uint32_t flags;                /* HVQ_F_* */
    uint32_t pic_kind, unk_shift;
    uint32_t width;                /* luma samples per row */
    uint32_t mcb_w, mcb_h;
    uint32_t total_tiles;
    uint32_t *q_offs;              /* self-referencing P pictures: the blocks' pool offsets, [(plane's first tile + tile) * HVQ_TILE_BLOCKS + block
                                      of the tile], where hvq_selfref_kernel looks for them; NULL otherwise */
    int has_nest;
    uint8_t nest[HVQ_NEST_BYTES];  /* unpacked by hvqd_view_set_nest */
} HvqdView;

/* the nibble-packed nest (HVQ_NESTP_BYTES) of a blob or a job record; NULL: the picture has none */
void hvqd_view_set_nest(HvqdView *v, const uint8_t *packed);
/* tiles of plane p */
uint32_t hvqd_view_plane_tiles(const HvqdView *v, int p);
/* reconstruct tile `tile` (0 = the plane's first) of plane p: HVQ_TILE_BLOCKS blocks in raster order.  In a self-referencing P picture
 * (q_offs set) the type-2 macroblocks' blocks are left out and every block's pool offset is stored for the walk. */
void hvqd_view_tile(const HvqdView *v, int p, uint32_t tile);
/* the raster-order walk of a self-referencing P picture: finished macroblocks move from `side` into `pic`, type-2 ones are computed from
 * `pic` as it is at that moment */
void hvqd_view_selfref(const HvqdView *v, const uint8_t *side, uint8_t *pic);

int hvqd_recon(const uint8_t *blob, uint8_t *dst, const uint8_t *ref0, const uint8_t *ref1, uint32_t slot_bytes);

#ifdef __cplusplus
}
#endif
#endif
