/*
 * hvq_desc.h -- per-picture descriptor blob: the interface between the host entropy
 * parse (hvq_parse.c) and the gfx950 reconstruction kernels (hvq_kernels.hip).
 *
 * The reference interleaves bit-buffer reads with pixel work (h4m_audio_decode.c:691, 726,
 * 1405-1406, 1950-1951).  Here the serial parse runs first and leaves everything the pixel
 * stage needs in one self-contained, position-independent blob (all offsets are byte offsets
 * from the blob start, every section 16-byte aligned):
 *
 *   HvqPicHeader
 *   map[3]      per plane (hb+2)*(vb+2) entries of {u8 value, u8 type} INCLUDING the border
 *               {0x7F,0xFF} -- byte-identical to the reference's BlockData maps (h4m:432-436,
 *               1001-1040).  I pictures: type = basis-count byte (luma) / nibble (chroma);
 *               P/B pictures: type = [6:5] macroblock type, [4] proc, [3:0] kind (h4m:1296-1304).
 *   mv          P/B only: per 8x8 macroblock {i16 ref_x, i16 ref_y}, the ABSOLUTE half-sample
 *               position of the macroblock in the reference picture (h4m:1954-1955); the
 *               predictor chain of getMVector (h4m:1846-1860) is resolved on the host.
 *   wave_base   one u32 per 64 blocks (HVQ_TILE_BLOCKS/64 per tile): dword index into `pool`
 *               of the first payload of that run of 64 blocks.
 *   pool        u32[]: block payloads in (plane, raster) order.  A block's payload length is a
 *               pure function of its map type (hvq_payload_dwords), so a wavefront finds each
 *               block's payload with one 64-lane prefix scan -- no per-block offsets are stored.
 *                 literal block (kind 6)      : 4 dwords = the 16 samples, row-major
 *                 AOT basis                   : 1 dword  = HVQ_BASIS(word, coef_sum)
 *                 MC-residual ("predi") block : 2 dwords {i32 dc_part, i32 gain_part} + bases
 *   nest        the 70x38 nest of 4-bit values packed two per byte (value n of the reference's
 *               nest_data[] = nibble n), HVQ_NESTP_BYTES; I pictures, and P/B pictures that contain
 *               intra AOT blocks (the nest of the most recent I picture, h4m:1823 -> 1367).
 *
 * A tile is HVQ_TILE_BLOCKS consecutive 4x4 blocks of ONE plane in raster order; one
 * workgroup reconstructs one tile.
 */
#ifndef HVQ_DESC_H
#define HVQ_DESC_H

#include <stddef.h>
#include <stdint.h>

#define HVQ_MAGIC        0x34515648u   /* "HVQ4" */
#ifndef HVQ_TILE_BLOCKS
#define HVQ_TILE_BLOCKS  256           /* blocks per tile = threads per workgroup */
#endif
#define HVQ_NEST_BYTES   (70 * 38)
#define HVQ_NESTP_BYTES  (HVQ_NEST_BYTES / 2 + 14)   /* nest packed two 4-bit values per byte, padded to 16 */

#define HVQ_PIC_I 0
#define HVQ_PIC_P 1
#define HVQ_PIC_B 2

/* header flags */
#define HVQ_F_IS15        0x0001u   /* HVQM4 1.5 stream: per-plane half-sample rule (h4m:1337-1343) */
#define HVQ_F_LANDSCAPE   0x0002u   /* width >= height (h4m:965-975) */
#define HVQ_F_HAS_NEST    0x0004u   /* blob carries a nest: some block needs intra AOT */
#define HVQ_F_SELF_REF    0x0008u   /* P picture with a future-referencing (type 2) macroblock: the reference
                                       reads the picture being written (h4m:2060).  Its other macroblocks are
                                       reconstructed data-parallel into a side buffer, then hvq_selfref_kernel walks the
                                       macroblocks in raster order like the reference does */
#define HVQ_F_BIG_AOT     0x0010u   /* some block has more than 15 bases (I-luma type byte > 15) */
#define HVQ_F_CLAMPED     0x0020u   /* malformed input the reference reads foreign memory on: a nest origin whose window leaves the block map or a
                                       vector target beyond 16 bits (clamped), a motion-compensated block or a sample of a used window basis
                                       outside [0, pic_bytes) of the referenced picture, anything read from a section of size 0 or a section
                                       whose size lies outside the picture (hvq_refuse.h) -- refused unless HVQM4_AMD_ALLOW_CLAMPED=1, under
                                       which the kernels pin every address into the slot and the picture is invented */
#define HVQ_F_CAPPED      0x0040u   /* an overflow-symbol loop (h4m:654-677: the reference sums for as long as the stream says) ended
                                       on this back end's cap instead of on the stream: the value differs from the reference's --
                                       the picture is refused, never decoded differently */
#define HVQ_F_MALFORMED   0x0080u   /* P/B picture the reference decodes outside its own rules: a luma kind symbol above 15 (it lands in
                                       the macroblock's type / proc bits, h4m:1701, 1927) or a type run that opens at value 3 (h4m:1591,
                                       1606, 1950-1951); in any picture, a prefix tree with more inner nodes than 256 leaf bytes allow
                                       (the device parser's GP_ST_BADTREE) -- refused, never decoded differently */

typedef struct HvqPicHeader {
    uint32_t magic;
    uint32_t total_bytes;
    uint16_t width, height;        /* luma samples */
    uint8_t  pic_kind;             /* HVQ_PIC_* */
    uint8_t  unk_shift;            /* h4m:1974 / 2022: accumulator scale of the AOT */
    uint8_t  dc_shift;             /* informational; already folded into pool values */
    uint8_t  wshift, hshift;       /* chroma subsampling shifts (1,1 for 4:2:0) */
    uint8_t  pad0[3];
    uint32_t flags;
    uint16_t hb[3], vb[3];         /* 4x4 blocks per plane */
    uint32_t plane_off[3];         /* byte offset of each plane inside a picture buffer */
    uint32_t pic_bytes;            /* Y|U|V size */
    uint32_t map_off[3];
    uint32_t mv_off;               /* 0 for I pictures */
    uint32_t wave_base_off;
    uint32_t pool_off;
    uint32_t pool_dwords;
    uint32_t nest_off;             /* 0 when absent */
    uint32_t tile_first[4];        /* first tile index of plane 0,1,2 and the total */
    uint32_t mcb_w, mcb_h;
    uint16_t max_items;            /* most queued (AOT) blocks in any tile: sizes the kernel's LDS accumulators */
    uint16_t pad1;
    uint32_t max_pairs;            /* most (block, basis) pairs in any tile */
    uint32_t reserved[3];
} HvqPicHeader;

#if defined(__cplusplus)
static_assert(sizeof(HvqPicHeader) == 128, "HvqPicHeader must be 128 bytes");
#else
_Static_assert(sizeof(HvqPicHeader) == 128, "HvqPicHeader must be 128 bytes");
#endif

/* AOT basis dword.  bits 12:0 = reference word bits 12:0 (offsets + strides, h4m:683-690),
 * bit 13 = negate (word bit 15), bits 31:14 = running coefficient sum + word offset bits 14:13
 * (the `*sum + offset` of h4m:726-731; <= 255*1020+3 < 2^18). */
#define HVQ_BASIS(word, sum_plus_off) \
    ((uint32_t)((word) & 0x1FFFu) | ((uint32_t)(((word) >> 15) & 1u) << 13) | ((uint32_t)(sum_plus_off) << 14))

/* Payload length in dwords of one block, from its map type byte.
 *   intra context (I picture, or P/B macroblock type 0; h4m:1433-1455, 1789-1827):
 *       kind 0 / 8 -> none; 6 -> literal; else -> `kind` bases
 *   inter context (h4m:1862-1910): proc = 1 -> none; kind 0 -> none; 6 -> literal;
 *       else -> 2 parameters + (kind-1) bases
 * `is_I_luma` selects the full type byte as kind (h4m:1093) instead of the low nibble. */
#if defined(__HIPCC__)
#define HVQ_HD __host__ __device__
#else
#define HVQ_HD
#endif
HVQ_HD static inline uint32_t hvq_payload_dwords(uint32_t type, int is_pb, int is_I_luma)
{
    /* written with selects only: the kernel evaluates it per lane */
    const uint32_t kind = is_I_luma ? type : (type & 0xFu);
    const int inter = is_pb && (type & 0x60u);
    const uint32_t n_intra = (kind == 0u || kind == 8u) ? 0u : kind;
    const uint32_t n_inter = ((type & 0x10u) || kind == 0u) ? 0u : kind + 1u;
    return kind == 6u ? ((inter && (type & 0x10u)) ? 0u : 4u) : (inter ? n_inter : n_intra);
}

/* one reconstruction job = one picture of one stream (device-visible).  Every member is a dword or a qword: the kernel reads
 * the record with scalar loads only (16-bit members would be fetched with vector loads), and because all tiles of a picture
 * read the SAME record it stays in the scalar cache / L2 -- unlike a per-tile record, whose first touch is an HBM miss
 * (~1.2-1.9k cycles, profiles/r02d). */
typedef struct HvqPlaneRec {       /* per-plane part (32 bytes) */
    uint64_t map;                  /* device address of the plane's map (entry [-1][-1], i.e. incl. border) */
    uint64_t dst;                  /* device address of the plane inside the destination picture */
    uint32_t plane_off;            /* byte offset of the plane inside a picture buffer (reference reads) */
    uint32_t tile_first;           /* first tile index of the plane */
    uint32_t hbvb;                 /* 4x4 blocks per row | rows << 16 */
    uint32_t pw_sub;               /* samples per row | ws << 16 | hs << 24 (subsampling shifts relative to luma) */
} HvqPlaneRec;

typedef struct HvqJob {                /* 232 bytes */
    uint64_t ring;                 /* the stream's picture slots: every reference read is ring + 32-bit offset (one SGPR base) */
    uint32_t ref0_off;             /* "past"   (macroblock type 1): byte offset of its slot inside the ring */
    uint32_t ref1_off;             /* "future" (macroblock type 2) */
    uint64_t pool;                 /* device addresses of the blob sections */
    uint64_t mv;
    uint64_t tq;                   /* HVQ_F_SELF_REF pictures: side section the level's launch leaves the blocks' pool offsets in (q_offs_off), else 0 */
    uint64_t nest;                 /* nibble-packed nest (HVQ_NESTP_BYTES), 0 when absent */
    uint32_t slot_bytes;           /* readable bytes of a slot (>= pic_bytes + 8) */
    uint32_t flags;                /* HVQ_F_* | picture kind << 16 | unk_shift << 20 */
    uint32_t width;                /* luma samples per row */
    uint32_t mcb_w;
    uint32_t pool_dwords;          /* payload pool size */
    uint32_t total_tiles;          /* 0: picture dropped by the flush, its workgroups exit */
    uint32_t tile_first12[2];      /* first tile of planes 1 and 2 (plane 0 starts at tile 0): a copy beside the common part, so that a workgroup knows its plane
                                      before it has loaded a plane record (the kernel addresses this record by dword index: dwords 18, 19) */
    HvqPlaneRec plane[3];
    uint32_t rsv1[2];
    uint64_t wave_base;            /* blob section: pool offset of every run of 64 blocks (scalar loads of hvq_recon_inline_kernel) */
    uint32_t rsv2;
    uint32_t q_offs_off;           /* HVQ_F_SELF_REF pictures: byte offset from `tq` of the blocks' pool offsets (u32 per block), else 0 */
    uint32_t pad2[2];
    uint32_t hb_magic[3];          /* per plane, hb = blocks per row: floor(2^32 / hb) + 1 (0 for hb = 1: the quotient is the index itself)
                                      -- mulhi(b, magic) is floor(b / hb) or one more for b < 2^22 (scalar split of a wave's first block) */
    uint32_t hb_magic16[3];        /* ceil(2^16 / hb): (t * magic16) >> 16 = floor(t / hb) exactly for t < 128 + hb, hb < 64 */
} HvqJob;
#define HVQ_JOB_KIND_SHIFT  16
#define HVQ_JOB_UNK_SHIFT   20

#if defined(__cplusplus)
static_assert(sizeof(HvqPlaneRec) == 32, "HvqPlaneRec must be 32 bytes");
static_assert(sizeof(HvqJob) == 232, "HvqJob must be 232 bytes");
#else
_Static_assert(sizeof(HvqPlaneRec) == 32, "HvqPlaneRec must be 32 bytes");
_Static_assert(sizeof(HvqJob) == 232, "HvqJob must be 232 bytes");
#endif

#define HVQ_PQ_NEG     (1u << 18)   /* a basis' gain word inside the kernel: coefficient sum + offset [17:0], negate */

/* launch table: one entry per picture of a launch.  The grid is (picture slots, tiles): consecutive workgroup ids differ in
 * the picture, and with the slot count a multiple of 8 all tiles of a picture run on one XCD (workgroups are dealt round-robin
 * over the 8 XCDs), keeping its map, nest and reference reads in that XCD's L2. */
typedef struct HvqTileRef {
    uint32_t job;                  /* 0xFFFFFFFF: padding slot */
    uint32_t tile;                 /* tiles of the picture */
} HvqTileRef;

/* one picture of the display epilogue / export (hvq_yuv_rgb_kernel): source planes of a slot, destination and its layout.
 * Output formats (HVQ_FMT_* of hvqm4_amd.h): 0 RGB24 interleaved rows of w*3 bytes, 1 RGB planar, 2 YUV 4:4:4 planar; planar
 * formats put three planes of h rows `plane_pitch` apart.  dst, row_pitch and plane_pitch are multiples of 4. */
typedef struct HvqRgbJob {
    const uint8_t *y, *u, *v;
    uint8_t *dst;
    int64_t row_pitch, plane_pitch;    /* bytes */
    int32_t w, h;
    int32_t wshift, hshift;            /* chroma subsampling: (1, 1) 4:2:0, (1, 0) 4:2:2, (0, 0) 4:4:4 */
} HvqRgbJob;

/* one picture of the float export (hvq_yuv_tensor_kernel): crop rectangle (x0, y0, cw, ch) of the source in luma samples, resized
 * to out_w x out_h, three planes `plane_pitch` bytes apart of out_h rows `row_pitch` bytes apart.  sx = cw / out_w and
 * sy = ch / out_h are divided on the host.  dst and the pitches are multiples of the element size.  112 bytes: tables are uploaded
 * in 16-byte units. */
#define HVQ_TJ_IDENT  1u            /* out size == crop size, loads and stores vectorised: the streaming body */
#define HVQ_TJ_VEC    2u            /* dst and pitches multiples of 16 bytes, out_w a multiple of the run length: 16-byte stores */
typedef struct HvqTensorJob {
    const uint8_t *y, *u, *v;
    uint8_t *dst;
    int64_t row_pitch, plane_pitch;    /* bytes */
    int32_t w, h;                      /* source picture */
    int32_t wshift, hshift;
    int32_t x0, y0, cw, ch;
    int32_t out_w, out_h;
    float sx, sy;
    uint32_t flags;
    uint32_t pad[3];
} HvqTensorJob;

/* per call: o = v * mul[c] + add[c] */
typedef struct HvqTensorNorm { float mul[3], add[3]; } HvqTensorNorm;

/* one picture of the antialiased float export (hvq_yuv_resample_kernel, hvq_export_resampled with HVQ_FILTER_TRIANGLE).  The weight
 * tables of the two axes lie behind the job records in the same upload; xtab / ytab are byte offsets from the table base (the end of
 * the records), multiples of 16.  One axis table of `n_out` outputs: int32 first[n_out] (first source index inside the crop),
 * int32 start[n_out + 1] (weights of output j are w[start[j] .. start[j + 1])), float w[start[n_out]], padded to 16 bytes.
 * Every member is a dword or a qword; 96 bytes: tables are uploaded in 16-byte units. */
#define HVQ_RJ_VEC    1u            /* dst and pitches multiples of 16 bytes, out_w a multiple of the run length: 16-byte stores */
#define HVQ_RJ_TILED  2u            /* a downscale whose largest tile footprint fits HVQ_RS_ROWS rows of LDS: the tiled body */
#define HVQ_RS_TILE_W 64            /* output columns of a tile */
#define HVQ_RS_ROWS   40            /* source rows of h the tiled body keeps in LDS: 3 * 40 * 64 floats = 30720 bytes per workgroup */
typedef struct HvqResampleJob {
    const uint8_t *y, *u, *v;
    uint8_t *dst;
    int64_t row_pitch, plane_pitch;    /* bytes */
    int32_t w;                         /* samples per luma row of the source picture */
    int32_t wshift, hshift;
    int32_t x0, y0;                    /* crop origin */
    int32_t out_w, out_h;
    int32_t tile_h;                    /* HVQ_RJ_TILED: output rows of a tile (16 or 8) */
    uint32_t xtab, ytab;
    uint32_t flags;
    uint32_t tiles_x;                  /* HVQ_RJ_TILED: tiles per tile row, ceil(out_w / HVQ_RS_TILE_W) */
} HvqResampleJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqResampleJob) == 96, "HvqResampleJob must be 96 bytes");
static_assert(sizeof(HvqResampleJob) % 16 == 0, "job tables are uploaded in 16-byte units");
static_assert(3 * HVQ_RS_ROWS * HVQ_RS_TILE_W * 4 == 30720, "five workgroups of the tiled body share a CU's 160 KiB of LDS");
#else
_Static_assert(sizeof(HvqResampleJob) == 96, "HvqResampleJob must be 96 bytes");
_Static_assert(sizeof(HvqResampleJob) % 16 == 0, "job tables are uploaded in 16-byte units");
#endif

/* one picture pair of the metrics launch (hvq_metrics_kernel, hvq_picture_metrics): picture `a` and its reference `b`, both Y|U|V tightly
 * packed (a slot, or the caller's memory in a slot's layout), and the output record uint64 [3 planes][4] = { sum_a, sum_b, sad, sse }
 * the launch adds into (zeroed in front of it).  b = 0: a reference of zeros, nothing is loaded for it.  A plane is units[p] 16-byte
 * units long (widths and heights are multiples of 8: every plane starts on a 16-byte boundary and is a multiple of 16 bytes); a
 * workgroup takes HVQ_MT_CHUNK consecutive units of ONE plane, wg_first[p] is the first workgroup of plane p (wg_first[0] = 0,
 * wg_first[3] = the picture's workgroups: those past it leave).  Every member is a dword or a qword (scalar loads); 64 bytes. */
#define HVQ_MT_LANES  256u          /* lanes of a workgroup */
#define HVQ_MT_UNITS  4u            /* 16-byte units of a lane, HVQ_MT_LANES apart: 64 samples of a and of b */
#define HVQ_MT_CHUNK  (HVQ_MT_LANES * HVQ_MT_UNITS)
typedef struct HvqMetricsJob {
    uint64_t a, b;                     /* device addresses, multiples of 16; b = 0: zeros */
    uint64_t out;                      /* device address of the record, a multiple of 8 */
    uint32_t plane_off[3];             /* byte offset of plane p inside a picture */
    uint32_t units[3];                 /* 16-byte units of plane p */
    uint32_t wg_first[4];
} HvqMetricsJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqMetricsJob) == 64, "HvqMetricsJob must be 64 bytes");
#else
_Static_assert(sizeof(HvqMetricsJob) == 64, "HvqMetricsJob must be 64 bytes");
#endif

/* one picture pair of the SSIM launch (hvq_ssim_kernel, hvq_picture_ssim): picture `a` and its reference `b`, both Y|U|V tightly packed, the
 * output record int64 [3 planes][2] = { sum_f, windows } the launch adds into (zeroed in front of it), and the pair's map of window values
 * (0: none).  Plane p is bw[p] x bh[p] blocks of 4 x 4 samples, rows 4 * bw[p] bytes apart, and has (bh[p] - 1) x (bw[p] - 1) windows; its
 * map starts map_off[p] floats into the pair's map.  A workgroup takes one tile of at most HVQ_SS_TR x HVQ_SS_TC windows of ONE plane, that
 * is (HVQ_SS_TR + 1) x (HVQ_SS_TC + 1) blocks; plane p has tiles_x[p] tiles per tile row, wg_first[p] is its first workgroup (wg_first[0]
 * = 0, wg_first[3] = the pair's workgroups: those past it leave).  A plane without a window (bw or bh below 2) has no workgroup.  Every
 * member is a dword or a qword (scalar loads); 112 bytes. */
#define HVQ_SS_LANES  256u          /* lanes of a workgroup */
#define HVQ_SS_TR     15u           /* window rows of a tile: 16 block rows */
#define HVQ_SS_TC     63u           /* window columns of a tile: 64 block columns */
typedef struct HvqSsimJob {
    uint64_t a, b;                     /* device addresses, multiples of 16 */
    uint64_t out;                      /* device address of the record, a multiple of 8 */
    uint64_t map;                      /* device address of the pair's map, a multiple of 4; 0: no map */
    uint32_t plane_off[3];             /* byte offset of plane p inside a picture */
    uint32_t map_off[3];               /* floats in front of plane p's windows inside the map */
    uint32_t bw[3], bh[3];             /* blocks per row, block rows */
    uint32_t tiles_x[3];
    uint32_t wg_first[4];
    uint32_t pad;
} HvqSsimJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqSsimJob) == 112, "HvqSsimJob must be 112 bytes");
static_assert(sizeof(HvqSsimJob) % 16 == 0, "job tables are uploaded in 16-byte units");
#else
_Static_assert(sizeof(HvqSsimJob) == 112, "HvqSsimJob must be 112 bytes");
_Static_assert(sizeof(HvqSsimJob) % 16 == 0, "job tables are uploaded in 16-byte units");
#endif

/* one picture of the checksum launch (hvq_checksum_kernel + hvq_checksum_finish_kernel, hvq_picture_checksums): picture `a`, Y|U|V tightly
 * packed (a slot, or the caller's memory in a slot's layout), its accumulator `acc` in library-owned memory, uint64 [3 planes][4] =
 * { R in the low dword, sum d, sum (len - i) d, unused } (hvq_checksum.h), zeroed in front of the launch, and the output record uint64 [8]
 * the finishing launch writes.  A plane is units[p] 16-byte units long; a workgroup takes HVQ_CK_CHUNK consecutive units of ONE plane,
 * counted from the plane's END (workgroup c of a plane has c whole chunks behind it; the one at the plane's start may be short: the units
 * in front of the plane are zeros, which leave a CRC register of 0 as it is).  wg_first as in HvqMetricsJob.  xlen[p] = x^(8 * bytes of
 * plane p) mod P, for the CRC's initial register and the picture value.  Every member is a dword or a qword (scalar loads); 80 bytes. */
#define HVQ_CK_LANES  256u          /* lanes of a workgroup */
#define HVQ_CK_UNITS  4u            /* 16-byte units of a lane, HVQ_CK_LANES apart */
#define HVQ_CK_CHUNK  (HVQ_CK_LANES * HVQ_CK_UNITS)
#define HVQ_CK_MAX_UNITS (1u << 22) /* 8192 x 8192 samples, the largest plane the library opens */
typedef struct HvqChecksumJob {
    uint64_t a;                        /* device address, a multiple of 16 */
    uint64_t acc;                      /* device address of the accumulator, a multiple of 8 */
    uint64_t out;                      /* device address of the record, a multiple of 8 */
    uint32_t plane_off[3];             /* byte offset of plane p inside a picture */
    uint32_t units[3];                 /* 16-byte units of plane p, at most HVQ_CK_MAX_UNITS */
    uint32_t wg_first[4];
    uint32_t xlen[3];
    uint32_t pad;
} HvqChecksumJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqChecksumJob) == 80, "HvqChecksumJob must be 80 bytes");
static_assert(sizeof(HvqChecksumJob) % 16 == 0, "job tables are uploaded in 16-byte units");
static_assert(offsetof(HvqChecksumJob, acc) == 8 && offsetof(HvqChecksumJob, out) == 16 && offsetof(HvqChecksumJob, plane_off) == 24 &&
              offsetof(HvqChecksumJob, units) == 36 && offsetof(HvqChecksumJob, wg_first) == 48 && offsetof(HvqChecksumJob, xlen) == 64,
              "the members hvq_checksum_kernel reads");
/* sum (len - i) d over a plane is at most 255 len (len + 1) / 2: an exact 64-bit integer for every plane the library opens */
static_assert(255ull * (16ull * HVQ_CK_MAX_UNITS) * (16ull * HVQ_CK_MAX_UNITS + 1ull) / 2ull < (1ull << 63), "Adler's weighted sum must fit 64 bits");
#else
_Static_assert(sizeof(HvqChecksumJob) == 80, "HvqChecksumJob must be 80 bytes");
#endif

/* one picture of the histogram launch (hvq_histogram_kernel, hvq_picture_histograms): picture `a` and, in HVQ_HIST_ABSDIFF, its reference
 * `b`, both Y|U|V tightly packed (a slot, or the caller's memory in a slot's layout), and the output record uint32 [3 planes][256] the
 * launch adds into (zeroed in front of it).  b = 0: HVQ_HIST_VALUES, bin v counts the samples of a equal to v; otherwise bin d counts
 * the positions where |a - b| = d.  A plane is units[p] 16-byte units long; a workgroup takes HVQ_HG_CHUNK consecutive units of ONE plane,
 * counts them in LDS and flushes its 256 bins once (1, 2, 4 and 8 chunks per workgroup were measured); wg_first as in HvqMetricsJob.
 * Every member is a dword or a qword (scalar loads); 64 bytes. */
#define HVQ_HG_BINS   256u          /* HVQ_HIST_BINS */
#define HVQ_HG_LANES  256u          /* lanes of a workgroup */
#define HVQ_HG_UNITS  4u            /* 16-byte units of a lane, HVQ_HG_LANES apart */
#define HVQ_HG_CHUNK  (HVQ_HG_LANES * HVQ_HG_UNITS)
#define HVQ_HG_MAX_UNITS (1u << 22) /* 8192 x 8192 samples, the largest plane the library opens */
typedef struct HvqHistogramJob {
    uint64_t a, b;                     /* device addresses, multiples of 16; b = 0: values of a */
    uint64_t out;                      /* device address of the record, a multiple of 4 */
    uint32_t plane_off[3];             /* byte offset of plane p inside a picture */
    uint32_t units[3];                 /* 16-byte units of plane p, at most HVQ_HG_MAX_UNITS */
    uint32_t wg_first[4];
} HvqHistogramJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqHistogramJob) == 64, "HvqHistogramJob must be 64 bytes");
static_assert(sizeof(HvqHistogramJob) % 16 == 0, "job tables are uploaded in 16-byte units");
static_assert(offsetof(HvqHistogramJob, b) == 8 && offsetof(HvqHistogramJob, out) == 16 && offsetof(HvqHistogramJob, plane_off) == 24 &&
              offsetof(HvqHistogramJob, units) == 36 && offsetof(HvqHistogramJob, wg_first) == 48, "the members hvq_histogram_kernel reads");
/* a bin holds at most the samples of its plane: 32 bits hold every count, in the record and (a workgroup's share) in LDS */
static_assert(16ull * HVQ_HG_MAX_UNITS == (1ull << 26) && 16ull * HVQ_HG_MAX_UNITS < (1ull << 32), "a 32-bit bin must hold the samples of the largest plane");
#else
_Static_assert(sizeof(HvqHistogramJob) == 64, "HvqHistogramJob must be 64 bytes");
#endif

/* one picture of the motion launch (hvq_motion_kernel, hvq_picture_motion): the luma planes of picture `a` and of its reference `b`, both
 * w x h bytes with pitch w, and the field int32 [rows][cols][4] = { dy, dx, cost, cost_zero } the launch writes, every record once with
 * one 16-byte store.  Block size and radius are those of the call (launch arguments).  A workgroup of HVQ_MV_LANES lanes takes one tile of
 * HVQ_MV_TILE x HVQ_MV_TILE samples of a, tiles_x tiles a row, tiles in all; it stages the tile's window of b, HVQ_MV_MAX_RADIUS at most
 * wider on every side, into LDS, and each of its waves searches blocks of the tile.  A candidate's key is
 * cost << 15 | (|dy| + |dx|) << 10 | (dy + R) << 5 | (dx + R): the smallest key is the winner of include/hvqm4_amd.h.
 * Every member is a dword or a qword (scalar loads); 48 bytes. */
#define HVQ_MV_LANES       256u     /* lanes of a workgroup */
#define HVQ_MV_TILE        64u      /* samples of a tile's side: a multiple of both block sizes */
#define HVQ_MV_MAX_RADIUS  15u      /* HVQ_MOTION_MAX_RADIUS */
#define HVQ_MV_MAX_SIDE    32768u   /* w and h stay below this: byte offsets inside a plane fit 30 bits */
typedef struct HvqMotionJob {
    uint64_t a, b;                     /* device addresses of the luma planes, multiples of 16 */
    uint64_t out;                      /* device address of the field, a multiple of 16 */
    uint32_t w, h;                     /* luma samples, multiples of the block */
    uint32_t rows, cols;               /* h / block, w / block */
    uint32_t tiles_x, tiles;           /* ceil(w / HVQ_MV_TILE), tiles_x * ceil(h / HVQ_MV_TILE) */
} HvqMotionJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqMotionJob) == 48, "HvqMotionJob must be 48 bytes");
static_assert(sizeof(HvqMotionJob) % 16 == 0, "job tables are uploaded in 16-byte units");
static_assert(offsetof(HvqMotionJob, b) == 8 && offsetof(HvqMotionJob, out) == 16 && offsetof(HvqMotionJob, w) == 24 && offsetof(HvqMotionJob, rows) == 32 &&
              offsetof(HvqMotionJob, tiles_x) == 40, "the members hvq_motion_kernel reads");
static_assert(HVQ_MV_TILE % 16u == 0 && HVQ_MV_TILE % 8u == 0, "a tile is made of whole blocks of either size");
/* the largest cost, 16 x 16 x 255, fits the 16 bits the key gives it, and the 16-bit lanes of v_qsad_pk_u16_u8 */
static_assert(16u * 16u * 255u < (1u << 16) && 2u * HVQ_MV_MAX_RADIUS < (1u << 5), "the key's fields hold their values");
#else
_Static_assert(sizeof(HvqMotionJob) == 48, "HvqMotionJob must be 48 bytes");
#endif

/* one picture of the three JPEG launches (hvq_jpeg.hip, hvq_encode_jpeg): the picture in slot layout (Y | U | V), the file's destination
 * with its capacity, where its length goes, and the picture's entries of the context's scratch: scr[scr_first] = 1 when the file fits its
 * capacity (written by the layout launch), scr[scr_first + 1 + j] = the stuffed byte length of restart interval j (written by the measure
 * launch), replaced by the interval's offset inside the file (layout launch), read by the emit launch.  A workgroup of HVQ_JP_LANES lanes
 * takes one restart interval (one MCU row: mw MCUs of hs * vs + 2 blocks), one lane a block, HVQ_JP_LANES / (hs * vs + 2) whole MCUs a
 * chunk.  The table is followed in the same upload by the quantisers of the call (HvqJpegQuant) and one header per distinct geometry
 * (HVQ_JPEG_HEADER_SLOT bytes each); hdr_off is the byte offset of this picture's header from the start of the table.
 * Every member is a dword or a qword (scalar loads); 64 bytes. */
#define HVQ_JP_LANES     128u       /* lanes of a workgroup of the measure and emit launches: blocks of a chunk */
#define HVQ_JP_MAX_SIDE  32768u     /* w and h stay below this */
typedef struct HvqJpegJob {
    uint64_t src;                      /* device address of the picture, a multiple of 16 */
    uint64_t out;                      /* device address of the file, a multiple of 16 */
    uint64_t cap;                      /* bytes at out */
    uint64_t len;                      /* device address of lengths[i], a multiple of 8 */
    uint32_t w, h;                     /* luma samples */
    uint32_t hs, vs;                   /* sampling factors of luma, 1 or 2 */
    uint32_t mw, mh;                   /* MCUs of a row, MCU rows = restart intervals */
    uint32_t scr_first;                /* first of the picture's mh + 1 dwords of scratch */
    uint32_t hdr_off;                  /* the picture's header, bytes from the start of the table */
} HvqJpegJob;

/* the quantisers of a call, hvq_jpeg_qpack of hvq_jpeg.h, [0] luminance and [1] chrominance, natural order */
typedef struct HvqJpegQuant { uint32_t q[2][64]; } HvqJpegQuant;

#if defined(__cplusplus)
static_assert(sizeof(HvqJpegJob) == 64 && sizeof(HvqJpegQuant) == 512, "HvqJpegJob must be 64 bytes, HvqJpegQuant 512");
static_assert(offsetof(HvqJpegJob, out) == 8 && offsetof(HvqJpegJob, cap) == 16 && offsetof(HvqJpegJob, len) == 24 && offsetof(HvqJpegJob, w) == 32 &&
              offsetof(HvqJpegJob, hs) == 40 && offsetof(HvqJpegJob, mw) == 48 && offsetof(HvqJpegJob, scr_first) == 56, "the members the JPEG kernels read");
#else
_Static_assert(sizeof(HvqJpegJob) == 64, "HvqJpegJob must be 64 bytes");
#endif

/* one picture of the two hash launches (hvq_phash.hip, hvq_picture_hashes): the luma plane `a` (w x h bytes, pitch w: the start of a slot,
 * or of the caller's memory in a slot's layout), the picture's cells `acc` in library-owned memory, uint64 [HVQ_PH_ROWS][HVQ_PH_COLS],
 * zeroed in front of the first launch, and the record uint64 [4] the finishing launch writes.  Cell (r, c) of acc is cell (r, c) of the
 * 32 x 32 grid for c < 32 and cell (r, c - 32) of the 32-row x 9-column grid for c >= 32 (include/hvqm4_amd.h: S8 and D follow from them).
 * A lane takes `cols` adjacent samples of a row (16, or 8 when w is no multiple of 16): a row has units = w / cols of them.  A workgroup of
 * HVQ_PH_LANES lanes takes cells_pw = 1, 2, 4 or 8 consecutive row cells, HVQ_PH_LANES / cells_pw = sub_lanes lanes each (a power of two:
 * lane l works on row cell l >> sub_shift of the workgroup's), and of every row HVQ_PH_LANES at most of its units: within a row cell lanes_x =
 * min(units, HVQ_PH_LANES) lanes stand side by side and rows_pp = sub_lanes / lanes_x rows deep (at least 1: cells_pw is 1 when a row fills the
 * workgroup).  Row cell r has the sample rows [h r / 32, ceil(h (r + 1) / 32)).  xchunks = ceil(units / HVQ_PH_LANES); workgroup g of the
 * picture has the row cells (g % (32 / cells_pw)) * cells_pw .. and chunk g / (32 / cells_pw); wgs = 32 / cells_pw * xchunks, those past it
 * leave.  Every member is a dword or a qword (scalar loads); 64 bytes. */
#define HVQ_PH_LANES  256u          /* lanes of a workgroup, of both launches */
#define HVQ_PH_ROWS   32u           /* row cells */
#define HVQ_PH_COLS   41u           /* column cells: 32 + 9 */
#define HVQ_PH_CELLS  (HVQ_PH_ROWS * HVQ_PH_COLS)
#define HVQ_PH_MAX_CPW 8u           /* most row cells of a workgroup */
#define HVQ_PH_MAX_SIDE 8192u       /* w and h stay at or below this: the widths of the accumulators (hvq_phash.hip) */
#define HVQ_PH_BATCH  4096u         /* pictures of one launch pair: the runtime cuts a larger call, its cells stay below 42 MiB */
typedef struct HvqHashJob {
    uint64_t a;                        /* device address of the luma plane, a multiple of 16 */
    uint64_t acc;                      /* device address of the cells, a multiple of 8 */
    uint64_t out;                      /* device address of the record, a multiple of 8 */
    uint32_t w, h;                     /* luma samples, multiples of 8 */
    uint32_t units, lanes_x;
    uint32_t rows_pp, wgs;
    uint32_t cells_pw, sub_shift;      /* row cells of a workgroup; log2 of the lanes of one */
    uint32_t pad[2];
} HvqHashJob;

/* hvq_hash_nearest: a workgroup of HVQ_HN_LANES lanes takes HVQ_HN_LANES queries, one a lane, and walks the database in tiles of HVQ_HN_TILE
 * hashes staged in LDS */
#define HVQ_HN_LANES  256u
#define HVQ_HN_TILE   1024u
#define HVQ_HN_MAX    (1u << 24)    /* HVQ_HASH_NEAREST_MAX: an index fits the low 24 bits of the key d << 24 | j */

#if defined(__cplusplus)
static_assert(sizeof(HvqHashJob) == 64, "HvqHashJob must be 64 bytes");
static_assert(sizeof(HvqHashJob) % 16 == 0, "job tables are uploaded in 16-byte units");
static_assert(offsetof(HvqHashJob, acc) == 8 && offsetof(HvqHashJob, out) == 16 && offsetof(HvqHashJob, w) == 24 && offsetof(HvqHashJob, units) == 32 &&
              offsetof(HvqHashJob, rows_pp) == 40 && offsetof(HvqHashJob, cells_pw) == 48, "the members the hash kernels read");
/* a cell is at most 255 w h: 64 bits hold it, 32 do not */
static_assert(255ull * HVQ_PH_MAX_SIDE * HVQ_PH_MAX_SIDE < (1ull << 34) && 255ull * HVQ_PH_MAX_SIDE * HVQ_PH_MAX_SIDE > (1ull << 32), "a cell needs 64 bits");
static_assert(HVQ_HN_TILE % HVQ_HN_LANES == 0, "every lane stages the same number of hashes of a tile");
#else
_Static_assert(sizeof(HvqHashJob) == 64, "HvqHashJob must be 64 bytes");
#endif


/* one plane of one picture of the scale launch (hvq_scale.hip, hvq_scale_pictures): three jobs a picture, Y, U, V.  `src` is the first
 * sample of the crop's part of the source plane (any byte address inside the picture: the picture itself starts and ends on a multiple of
 * 16, and pitch is a multiple of 4, so the dwords around a row of the crop lie inside the picture), ny rows of nx samples, `pitch` bytes
 * from row to row; `dst` is the target plane, my rows of mx samples, dense (pitch mx: a multiple of 4, as dst is).  The values are
 * include/hvqm4_amd.h's: out = (S + (D >> 1)) / D with D = nx ny, as the high 64 bits of (S + (D >> 1)) * magic, magic = ceil(2^64 / D)
 * (hvq_scale.h: why that is exact).  Grid row = picture, its three jobs one behind the other; a workgroup of HVQ_SC_LANES lanes takes a
 * tile of one plane -- HVQ_SC_TW x HVQ_SC_TH target samples in the tiled body, HVQ_SC_DTW x HVQ_SC_DTH in the direct one: tiles_x tiles
 * side by side, `tiles` in all; the workgroups of a grid row walk the tiles of Y, then U, then V, those past them leave.  body
 * HVQ_SC_DIRECT: a lane computes four adjacent samples in each of four rows from global memory (at most 2 x 2 taps each when chosen).  body HVQ_SC_TILED: the tile's source rows go through LDS, `chunk` rows at a
 * time, `row_dwords` dwords a row (the most a tile of this plane needs); horizontal sums of a chunk once (32 bits: at most 255 nx <
 * 2^21), then the vertical pass into cells of 32 bits when 255 nx ny < 2^32 and of 64 bits (HVQ_SC_WIDE) otherwise.  The first and last
 * source of a target, floor(n r / m) and ceil(n (r + 1) / m), are a multiplication and a shift with mul_x / mul_y.  Every member is a dword
 * or a qword (scalar loads); 80 bytes. */
#define HVQ_SC_LANES  256u
#define HVQ_SC_TW     64u           /* target samples a tile is wide: 16 dwords, one store a lane and row */
#define HVQ_SC_TH     16u           /* target rows of a tile */
#define HVQ_SC_DTW    256u          /* the direct body's tile: a wave stores 256 adjacent bytes of a row, a lane four rows 4 apart */
#define HVQ_SC_DTH    16u
#define HVQ_SC_RAW_DWORDS 4096u     /* LDS of the staged source rows of a chunk */
#define HVQ_SC_MAX_CHUNK 32u        /* most source rows of a chunk */
#define HVQ_SC_MAX_RATIO 32u        /* n <= 32 m per plane and axis */
#define HVQ_SC_DIRECT 0u
#define HVQ_SC_TILED  1u
#define HVQ_SC_WIDE   2u
typedef struct HvqScaleJob {
    uint64_t src;                      /* device address of the first sample of the crop in the source plane */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    uint64_t magic;                    /* ceil(2^64 / (nx ny)) */
    uint32_t pitch;                    /* bytes between source rows, a multiple of 4 */
    uint32_t nx, ny;                   /* source samples of the crop */
    uint32_t mx, my;                   /* target samples: mx a multiple of 4 */
    uint32_t tiles_x, tiles;
    uint32_t body;                     /* HVQ_SC_DIRECT or HVQ_SC_TILED, | HVQ_SC_WIDE: cells of 64 bits */
    uint32_t chunk, row_dwords;        /* the tiled body's: chunk * row_dwords <= HVQ_SC_RAW_DWORDS, 1 <= chunk <= HVQ_SC_MAX_CHUNK */
    uint32_t mul_x, shift_x;           /* v / mx = v * mul_x >> shift_x for v < 2^27 (hvq_scale.h): no lane divides */
    uint32_t mul_y, shift_y;           /* likewise by my */
} HvqScaleJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqScaleJob) == 80 && sizeof(HvqScaleJob) % 16 == 0, "HvqScaleJob must be 80 bytes: job tables are uploaded in 16-byte units");
static_assert(offsetof(HvqScaleJob, dst) == 8 && offsetof(HvqScaleJob, magic) == 16 && offsetof(HvqScaleJob, pitch) == 24 && offsetof(HvqScaleJob, tiles_x) == 44 &&
              offsetof(HvqScaleJob, body) == 52 && offsetof(HvqScaleJob, chunk) == 56 && offsetof(HvqScaleJob, mul_x) == 64 && offsetof(HvqScaleJob, mul_y) == 72, "the members the scale kernel reads");
static_assert(HVQ_SC_TW * HVQ_SC_TH == HVQ_SC_LANES * 4u, "a lane stores one dword of the tile");
static_assert(HVQ_SC_DTW == 64u * 4u && HVQ_SC_DTH * 64u == HVQ_SC_LANES * 4u, "the direct body: 64 lanes side by side, four waves, four rows a lane");
static_assert(HVQ_SC_MAX_CHUNK == 32u, "a wave stages eight rows of a chunk, all loads issued before the first is used");
/* the widest row of a tile: 64 targets at 32 sources each, one more at each edge, three bytes of alignment in front, rounded up */
static_assert((HVQ_SC_TW * HVQ_SC_MAX_RATIO + 2u + 3u + 3u) / 4u <= HVQ_SC_RAW_DWORDS, "a chunk holds one row at least");
#else
_Static_assert(sizeof(HvqScaleJob) == 80, "HvqScaleJob must be 80 bytes");
#endif


/* one plane of one picture of the filter launch (hvq_filter.hip, hvq_filter_pictures): three jobs a picture, Y, U, V.  `src` and `dst`
 * are planes of ny rows of nx samples, dense (pitch nx: a multiple of 4, as both addresses are).  `pf` names the plane's record in the
 * table of HvqFilterPlaneDev that lies behind the job table in the same upload: 2 * filter for Y, 2 * filter + 1 for U and V.  Grid row
 * = picture, its three jobs one behind the other; a workgroup of HVQ_FL_LANES lanes takes a tile of one plane -- HVQ_FL_TW x HVQ_FL_TH
 * samples in the filter body, HVQ_FL_CTW x HVQ_FL_CTH in the copy body (a plane whose filter is the identity): tiles_x tiles side by
 * side, `tiles` in all; the workgroups of a grid row walk the tiles of Y, then U, then V, those past them leave.  Every member is a
 * dword or a qword (scalar loads); 48 bytes. */
#define HVQ_FL_LANES  256u
#define HVQ_FL_TW     64u           /* samples a tile of the filter body is wide: 16 dwords, one store a lane */
#define HVQ_FL_TH     16u           /* its rows */
#define HVQ_FL_CTW    256u          /* the copy body's tile: a wave moves 256 adjacent bytes of a row, a lane four rows 4 apart */
#define HVQ_FL_CTH    16u
#define HVQ_FL_MAX_R  15u           /* the largest radius: HVQ_FLT_MAX_RADIUS */
#define HVQ_FL_HALO   16u           /* bytes staged left and right of a tile's 64: the radius rounded up to whole dwords */
#define HVQ_FL_ROW_DWORDS ((HVQ_FL_TW + 2u * HVQ_FL_HALO) / 4u)   /* 24 */
#define HVQ_FL_MAX_ROWS (HVQ_FL_TH + 2u * HVQ_FL_MAX_R)          /* 46 staged rows at the most */
#define HVQ_FL_FILTER 0u
#define HVQ_FL_COPY   1u
typedef struct HvqFilterJob {
    uint64_t src;                      /* device address of the source plane, a multiple of 4 */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    uint32_t nx, ny;                   /* samples of the plane: nx a multiple of 4 */
    uint32_t tiles_x, tiles;
    uint32_t pf;                       /* index of the plane's HvqFilterPlaneDev */
    uint32_t body;                     /* HVQ_FL_FILTER or HVQ_FL_COPY */
    uint32_t pad[2];
} HvqFilterJob;

/* a plane's filter as the kernel reads it: include/hvqm4_amd.h's HvqPlaneFilter with the taps widened to dwords, so that a tap is one
 * scalar load.  Taps past 2 r + 1 are 0.  rmax = max(ry) over the terms: the rows staged above and below a tile. */
typedef struct HvqFilterTermDev { int32_t rx, ry; int32_t wx[32], wy[32]; } HvqFilterTermDev;
typedef struct HvqFilterPlaneDev {
    int32_t terms, combine, shift, bias;
    int32_t half, rmax, pad[2];        /* half = shift ? 1 << (shift - 1) : 0 */
    HvqFilterTermDev term[2];
} HvqFilterPlaneDev;

#if defined(__cplusplus)
static_assert(sizeof(HvqFilterJob) == 48 && sizeof(HvqFilterJob) % 16 == 0, "HvqFilterJob must be 48 bytes: job tables are uploaded in 16-byte units");
static_assert(sizeof(HvqFilterTermDev) == 264 && sizeof(HvqFilterPlaneDev) == 560 && sizeof(HvqFilterPlaneDev) % 16 == 0, "the filter table is uploaded in 16-byte units");
static_assert(HVQ_FL_TW * HVQ_FL_TH == HVQ_FL_LANES * 4u, "a lane stores one dword of the tile");
static_assert(HVQ_FL_CTW == 64u * 4u && HVQ_FL_CTH * 64u == HVQ_FL_LANES * 4u, "the copy body: 64 lanes side by side, four waves, four rows a lane");
static_assert(HVQ_FL_HALO >= HVQ_FL_MAX_R && HVQ_FL_HALO % 4u == 0 && HVQ_FL_TW % 4u == 0, "the staged row: whole dwords that hold the halo");
static_assert(HVQ_FL_MAX_ROWS * HVQ_FL_ROW_DWORDS <= 5u * HVQ_FL_LANES, "a lane stages five dwords at the most");
#else
_Static_assert(sizeof(HvqFilterJob) == 48, "HvqFilterJob must be 48 bytes");
#endif


/* one plane of one picture of the warp launch (hvq_warp.hip, hvq_warp_pictures): three jobs a picture, Y, U, V.  `src` is the source
 * plane, ny rows of nx samples, `dst` the target plane, my rows of mx samples, both dense (pitches nx and mx: multiples of 4, as both
 * addresses are).  The plane's inverse map in the units of include/hvqm4_amd.h: NU(x, y) = cu + au x + bu y and NV(x, y) = cv + av x +
 * bv y (au = 2 m00 hx', bu = 2 m01 vy', cu = m00 hx' + m01 vy' + 2 t0 - 65536 hx, ...), U8 = (NU + (1 << (su - 1))) >> su with su = 8 + hx,
 * sv = 8 + vy.  Grid row = picture, its three jobs one behind the other; a workgroup of HVQ_WP_LANES lanes takes a tile of HVQ_WP_TW x
 * HVQ_WP_TH targets of one plane: tiles_x tiles side by side, `tiles` in all; the workgroups of a grid row walk the tiles of Y, then U,
 * then V, those past them leave.  body HVQ_WP_DIRECT: a lane gathers its taps from global memory.  body HVQ_WP_TILED: the source
 * bounding box of the tile (hvq_warp.h), clamped into the plane, is staged into LDS as aligned dwords, `pitch` dwords a row (odd: lanes
 * that walk down a column of the box meet different banks) and at most `rows` rows, pitch * rows <= HVQ_WP_LDS_DWORDS; staged dword
 * idx is row idx / pitch = idx * pitch_mul >> 32.  Every member is a dword or a qword (scalar loads); 112 bytes. */
#define HVQ_WP_LANES  256u
#define HVQ_WP_TW     64u           /* targets a tile is wide: 16 dwords, one store a lane */
#define HVQ_WP_TH     16u           /* its rows: a lane computes four, 4 g .. 4 g + 3 for wave g */
#define HVQ_WP_LDS_DWORDS 4096u     /* LDS of the staged box: 16 KiB, beside 1 KiB for the tile's bytes */
#define HVQ_WP_DIRECT 0u
#define HVQ_WP_TILED  1u
#define HVQ_WP_MAX_M  (32 * 65536)  /* HVQ_WARP_MAX_SCALE */
typedef struct HvqWarpJob {
    uint64_t src;                      /* device address of the source plane, a multiple of 4 */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    int64_t  cu, cv;                   /* NU, NV of target sample (0, 0) */
    int32_t  au, bu, av, bv;           /* NU, NV from one target column / row to the next: |.| <= 2^23 */
    uint32_t nx, ny;                   /* source samples: nx a multiple of 4 */
    uint32_t mx, my;                   /* target samples: mx a multiple of 4 */
    uint32_t tiles_x, tiles;
    uint32_t body;                     /* HVQ_WP_DIRECT or HVQ_WP_TILED */
    uint32_t su, sv;                   /* 9 or 10 */
    uint32_t border, fill;             /* HVQ_WARP_REPLICATE / HVQ_WARP_CONSTANT; the plane's fill value */
    uint32_t pitch, rows;              /* the tiled body's */
    uint32_t pitch_mul;                /* floor(2^32 / pitch) + 1 */
    uint32_t pad[2];
} HvqWarpJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqWarpJob) == 112 && sizeof(HvqWarpJob) % 16 == 0, "HvqWarpJob must be 112 bytes: job tables are uploaded in 16-byte units");
static_assert(HVQ_WP_TW * HVQ_WP_TH == HVQ_WP_LANES * 4u && HVQ_WP_TW == 64u, "a lane stores one dword of the tile; a wave is a row of targets");
/* the deltas of NU inside a tile stay in 32 bits: 2 * 2 * HVQ_WP_MAX_M * (63 + 15) < 2^31 */
static_assert((int64_t)4 * HVQ_WP_MAX_M * (HVQ_WP_TW - 1u + HVQ_WP_TH - 1u) < ((int64_t)1 << 31), "a lane adds a 32-bit delta to the tile's origin");
#else
_Static_assert(sizeof(HvqWarpJob) == 112, "HvqWarpJob must be 112 bytes");
#endif


/* the compose launch (hvq_compose.hip, hvq_compose_pictures): three HvqComposeJob a target, Y, U, V, and behind the jobs of all targets,
 * in the same upload, three HvqComposeRec a layer, Y, U, V: record 3 l + p is plane p of layer l of the call.  A job names its layers
 * as the call does: layers first .. first + count - 1, in that order.  `dst` is the target plane, my rows of mx samples, dense (pitch
 * mx: a multiple of 4, as the address is).  A record holds the layer's two rectangles in samples of its plane: the w x h samples whose
 * first one is (sx, sy) of the source plane (`src`, ny rows of `pitch` samples, dense; pitch a multiple of 4, as the address is) land
 * at (dx, dy) of the target plane.  Grid row = target; a workgroup of HVQ_CP_LANES lanes takes a tile of HVQ_CP_TW x HVQ_CP_TH targets
 * of one plane, a lane one dword of it: tiles_x tiles side by side, `tiles` in all; the workgroups of a grid row walk the tiles of Y,
 * then U, then V, those past them leave.  body HVQ_CP_ALIGNED: dx, w and sx - dx are multiples of 4, a target dword is covered whole or
 * not at all and takes one aligned source dword.  body HVQ_CP_GENERAL: any offset, a cover mask per byte, the four source bytes from
 * the two aligned dwords that hold them.  Every member is a dword or a qword (scalar loads). */
#define HVQ_CP_LANES  256u
#define HVQ_CP_TW     64u           /* targets a tile is wide: 16 dwords, one store a lane */
#define HVQ_CP_TH     16u           /* its rows: lane l owns dword l & 15 of row l >> 4 */
#define HVQ_CP_ALIGNED 0u
#define HVQ_CP_GENERAL 1u
#define HVQ_CP_PUT    0u            /* HVQ_CMP_PUT */
#define HVQ_CP_ADD    1u            /* HVQ_CMP_ADD */
#define HVQ_CP_MAX_GAIN (1 << 22)   /* HVQ_CMP_MAX_GAIN */
typedef struct HvqComposeJob {
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    uint32_t mx, my;                   /* target samples: mx a multiple of 4 */
    uint32_t tiles_x, tiles;
    uint32_t first, count;             /* the target's layers, in layers of the call */
    int32_t  shift, half, bias;        /* half = shift ? 1 << (shift - 1) : 0 */
    uint32_t plane;                    /* 0: Y, 1: U, 2: V: which record of a layer */
} HvqComposeJob;
typedef struct HvqComposeRec {
    uint64_t src;                      /* device address of the source plane, a multiple of 4 */
    uint32_t pitch, ny;                /* the source plane: ny rows of pitch samples, pitch a multiple of 4 */
    int32_t  sx, sy;                   /* the rectangle's first sample in the source plane */
    int32_t  dx, dy;                   /* where it lands in the target plane */
    int32_t  w, h;                     /* its samples, both at least 1 */
    int32_t  weight;                   /* |weight| <= HVQ_CP_MAX_GAIN */
    uint32_t mode;                     /* HVQ_CP_PUT or HVQ_CP_ADD */
    uint32_t body;                     /* HVQ_CP_ALIGNED or HVQ_CP_GENERAL */
    uint32_t pad[3];
} HvqComposeRec;

#if defined(__cplusplus)
static_assert(sizeof(HvqComposeJob) == 48 && sizeof(HvqComposeRec) == 64, "job tables are uploaded in 16-byte units");
static_assert(HVQ_CP_TW * HVQ_CP_TH == HVQ_CP_LANES * 4u && HVQ_CP_TW == 64u, "a lane owns one dword of the tile");
/* |acc| + half <= 255 * 2^22 + 2^21 < 2^31: 32-bit signed arithmetic serves; a weight fits the 24-bit multiplier */
static_assert((int64_t)255 * HVQ_CP_MAX_GAIN + (HVQ_CP_MAX_GAIN >> 1) < ((int64_t)1 << 31) && HVQ_CP_MAX_GAIN < (1 << 23), "the accumulators are 32 bits");
#else
_Static_assert(sizeof(HvqComposeJob) == 48, "HvqComposeJob must be 48 bytes");
#endif


/* one plane of one picture of the rank launch (hvq_rank.hip, hvq_rank_pictures): three jobs a picture, Y, U, V.  `src` and `dst` are
 * planes of ny rows of nx samples, dense (pitch nx: a multiple of 4, as both addresses are).  The plane's operation and radii stand in
 * the job itself: there is no table behind the jobs.  Grid row = picture, its three jobs one behind the other; a workgroup of
 * HVQ_RK_LANES lanes takes a tile of one plane -- HVQ_RK_TW x HVQ_RK_TH targets in the min/max and median bodies, HVQ_RK_CTW x
 * HVQ_RK_CTH in the copy body: tiles_x tiles side by side, `tiles` in all; the workgroups of a grid row walk the tiles of Y, then U, then
 * V, those past them leave.  Every member is a dword or a qword (scalar loads); 48 bytes. */
#define HVQ_RK_LANES  256u
#define HVQ_RK_TW     64u           /* targets a tile is wide: 16 dwords, one store a lane */
#define HVQ_RK_TH     16u           /* its rows: lane l owns dword l & 15 of row l >> 4 */
#define HVQ_RK_CTW    256u          /* the copy body's tile: a wave moves 256 adjacent bytes of a row, a lane four rows 4 apart */
#define HVQ_RK_CTH    16u
#define HVQ_RK_MAX_R  15u           /* the largest radius: HVQ_RNK_MAX_RADIUS */
#define HVQ_RK_HALO   16u           /* bytes staged left and right of a tile's 64: the radius rounded up to whole dwords */
#define HVQ_RK_ROW_DWORDS ((HVQ_RK_TW + 2u * HVQ_RK_HALO) / 4u)   /* 24 */
#define HVQ_RK_MAX_ROWS (HVQ_RK_TH + 2u * HVQ_RK_MAX_R)          /* 46 staged rows at the most */
#define HVQ_RK_BUF    (HVQ_RK_MAX_ROWS * HVQ_RK_ROW_DWORDS)      /* dwords of one of the five LDS arrays */
#define HVQ_RK_SORTED (HVQ_RK_TH * HVQ_RK_ROW_DWORDS)            /* dwords of one level of the medians' sorted columns */
#define HVQ_RK_COPY   0u
#define HVQ_RK_MINMAX 1u
#define HVQ_RK_MED3   2u
#define HVQ_RK_MED5   3u
typedef struct HvqRankJob {
    uint64_t src;                      /* device address of the source plane, a multiple of 4 */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    uint32_t nx, ny;                   /* samples of the plane: nx a multiple of 4 */
    uint32_t tiles_x, tiles;
    uint32_t body;                     /* HVQ_RK_COPY, HVQ_RK_MINMAX, HVQ_RK_MED3 or HVQ_RK_MED5 */
    uint32_t op;                       /* HVQ_RNK_MIN, MAX or RANGE for the min/max body (a median of radius 0 runs it as MIN) */
    uint32_t rx, ry;                   /* the radii, 0 .. HVQ_RK_MAX_R */
} HvqRankJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqRankJob) == 48 && sizeof(HvqRankJob) % 16 == 0, "HvqRankJob must be 48 bytes: job tables are uploaded in 16-byte units");
static_assert(HVQ_RK_TW * HVQ_RK_TH == HVQ_RK_LANES * 4u && HVQ_RK_TW == 64u, "a lane stores one dword of the tile");
static_assert(HVQ_RK_CTW == 64u * 4u && HVQ_RK_CTH * 64u == HVQ_RK_LANES * 4u, "the copy body: 64 lanes side by side, four waves, four rows a lane");
static_assert(HVQ_RK_HALO >= HVQ_RK_MAX_R + 1u && HVQ_RK_HALO % 4u == 0, "the staged row: whole dwords that hold the halo; an unaligned read takes the dword behind");
static_assert(HVQ_RK_BUF <= 5u * HVQ_RK_LANES && HVQ_RK_MAX_ROWS * 16u <= 3u * HVQ_RK_LANES, "a lane takes five dwords of a staged array, three of a tile-wide one");
static_assert(5u * HVQ_RK_SORTED <= 4u * HVQ_RK_BUF && HVQ_RK_SORTED <= 2u * HVQ_RK_LANES, "the sorted columns of the 5 x 5 median fit behind the staged rows");
#else
_Static_assert(sizeof(HvqRankJob) == 48, "HvqRankJob must be 48 bytes");
#endif


/* one plane of one picture of the bilateral launch (hvq_bilateral.hip, hvq_bilateral_pictures): three jobs a picture, Y, U, V.  `src`,
 * `dst` and `guide` are planes of ny rows of nx samples, dense (pitch nx: a multiple of 4, as the addresses are); guide is 0 where the
 * plane guides itself.  Behind the jobs of a launch lie the call's parameter sets as they stand in include/hvqm4_amd.h, luma and chroma
 * of set 0, of set 1, ...: `ps` is the index of the plane's HvqBilateralPlane among them (HVQ_BL_PLANE_BYTES each; the kernel reads its
 * `spatial` rows as qwords and copies its `range` bytes into LDS).  Grid row = picture, its three jobs one behind the other; a workgroup
 * of HVQ_BL_LANES lanes takes a tile of one plane -- HVQ_BL_TW x HVQ_BL_TH targets in the general body, HVQ_BL_CTW x HVQ_BL_CTH in the
 * copy body: tiles_x tiles side by side, `tiles` in all; the workgroups of a grid row walk the tiles of Y, then U, then V, those past
 * them leave.  Every member is a dword or a qword (scalar loads); 64 bytes. */
#define HVQ_BL_LANES  256u
#define HVQ_BL_TW     64u           /* targets a tile is wide: 16 dwords, one store a lane */
#define HVQ_BL_TH     16u           /* its rows: lane l owns dword l & 15 of row l >> 4 */
#define HVQ_BL_CTW    256u          /* the copy body's tile: a wave moves 256 adjacent bytes of a row, a lane four rows 4 apart */
#define HVQ_BL_CTH    16u
#define HVQ_BL_MAX_R  7u            /* the largest radius: HVQ_BIL_MAX_RADIUS */
#define HVQ_BL_HALO   8u            /* bytes staged left and right of a tile's 64: the radius rounded up to whole dwords */
#define HVQ_BL_ROW_DWORDS ((HVQ_BL_TW + 2u * HVQ_BL_HALO) / 4u)   /* 20 */
#define HVQ_BL_MAX_ROWS (HVQ_BL_TH + 2u * HVQ_BL_MAX_R)          /* 30 staged rows at the most */
#define HVQ_BL_BUF    (HVQ_BL_MAX_ROWS * HVQ_BL_ROW_DWORDS)      /* dwords of a staged tile: the source's, and the guide's */
#define HVQ_BL_PLANE_BYTES 336u     /* sizeof(HvqBilateralPlane): rx, ry, pad[2], spatial[8][8], range[256] */
#define HVQ_BL_SPATIAL_AT  16u      /* ... the byte its spatial table begins at */
#define HVQ_BL_RANGE_AT    80u      /* ... and its range table */
#define HVQ_BL_COPY    0u
#define HVQ_BL_GENERAL 1u
typedef struct HvqBilateralJob {
    uint64_t src;                      /* device address of the source plane, a multiple of 4 */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    uint64_t guide;                    /* device address of the guide plane, a multiple of 4; 0: the source guides itself */
    uint32_t nx, ny;                   /* samples of the plane: nx a multiple of 4 */
    uint32_t tiles_x, tiles;
    uint32_t body;                     /* HVQ_BL_COPY or HVQ_BL_GENERAL */
    uint32_t ps;                       /* index of the plane's HvqBilateralPlane behind the jobs */
    uint32_t rx, ry;                   /* the radii, 0 .. HVQ_BL_MAX_R */
    uint32_t pad[2];
} HvqBilateralJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqBilateralJob) == 64 && sizeof(HvqBilateralJob) % 16 == 0, "HvqBilateralJob must be 64 bytes: job tables are uploaded in 16-byte units");
static_assert(HVQ_BL_TW * HVQ_BL_TH == HVQ_BL_LANES * 4u && HVQ_BL_TW == 64u, "a lane stores one dword of the tile");
static_assert(HVQ_BL_CTW == 64u * 4u && HVQ_BL_CTH * 64u == HVQ_BL_LANES * 4u, "the copy body: 64 lanes side by side, four waves, four rows a lane");
static_assert(HVQ_BL_HALO >= HVQ_BL_MAX_R + 1u && HVQ_BL_HALO % 4u == 0, "the staged row: whole dwords that hold the halo; an unaligned read takes the dword behind");
static_assert(HVQ_BL_BUF <= 3u * HVQ_BL_LANES, "a lane stages three dwords of a tile at the most");
static_assert(HVQ_BL_PLANE_BYTES % 16u == 0 && HVQ_BL_SPATIAL_AT % 8u == 0 && HVQ_BL_RANGE_AT % 4u == 0, "the sets lie behind the jobs in 16-byte units; rows of qwords, a table of dwords");
#else
_Static_assert(sizeof(HvqBilateralJob) == 64, "HvqBilateralJob must be 64 bytes");
#endif


/* one plane of one picture of the map launch (hvq_map.hip, hvq_map_pictures): three jobs a picture, Y, U, V.  A point operation does not
 * look at rows: `src` and `dst` are the plane's `dwords` dwords, dense.  `table` is the device address of the plane's 256 table bytes
 * (a multiple of 16: record which[i], plane p); a plane that is copied (its bit of `planes` is clear) has body HVQ_MP_COPY and table 0.
 * Grid row = picture, its three jobs one behind the other; a workgroup of HVQ_MP_LANES lanes takes a tile of HVQ_MP_TILE consecutive
 * dwords of one plane, a lane HVQ_MP_PER dwords HVQ_MP_LANES apart: the workgroups of a grid row walk the tiles of Y, then U, then V, those
 * past them leave.  Every member is a dword or a qword (scalar loads); 48 bytes. */
#define HVQ_MP_LANES  256u
#define HVQ_MP_PER    8u
#define HVQ_MP_TILE   (HVQ_MP_LANES * HVQ_MP_PER)     /* 2048 dwords = 8 KiB of a plane: 32 bytes looked up for every table byte staged */
#define HVQ_MP_COPY   0u
#define HVQ_MP_LOOKUP 1u
typedef struct HvqMapJob {
    uint64_t src;                      /* device address of the source plane, a multiple of 4 */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4; may equal src */
    uint64_t table;                    /* device address of the plane's uint8 [256], a multiple of 16 (0 in the copy body) */
    uint32_t dwords;                   /* dwords of the plane */
    uint32_t tiles;                    /* ceil(dwords / HVQ_MP_TILE) */
    uint32_t body;                     /* HVQ_MP_COPY or HVQ_MP_LOOKUP */
    uint32_t pad[3];
} HvqMapJob;

/* one histogram record of the table launch (hvq_map.hip, hvq_histogram_tables): grid row = record, grid column = plane; a workgroup of
 * HVQ_TB_LANES lanes, lane v holding bin v, writes the plane's 256 table bytes.  rule[0] serves Y, rule[1] U and V.  48 bytes. */
#define HVQ_TB_LANES 256u
typedef struct HvqTableJob {
    uint64_t hist;                     /* device address of the record, uint32 [3][256], a multiple of 16 */
    uint64_t out;                      /* device address of the table record, uint8 [3][256], a multiple of 16 */
    struct { uint32_t kind, a, b, pad; } rule[2];
} HvqTableJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqMapJob) == 48 && sizeof(HvqMapJob) % 16 == 0, "HvqMapJob must be 48 bytes: job tables are uploaded in 16-byte units");
static_assert(sizeof(HvqTableJob) == 48 && sizeof(HvqTableJob) % 16 == 0, "HvqTableJob must be 48 bytes: job tables are uploaded in 16-byte units");
static_assert(HVQ_MP_LANES == 256u && HVQ_TB_LANES == 256u, "a lane stages one table byte; lane v holds bin v");
#else
_Static_assert(sizeof(HvqMapJob) == 48, "HvqMapJob must be 48 bytes");
_Static_assert(sizeof(HvqTableJob) == 48, "HvqTableJob must be 48 bytes");
#endif

/* one picture of the label launches (hvq_label.hip, hvq_label_pictures): the plane of the picture's rule, its label map and its record
 * table.  Grid row = picture in every launch.  A tile is HVQ_LB_TX x HVQ_LB_TY samples, a workgroup of HVQ_LB_LANES lanes labels it in
 * LDS, a lane four samples of a row (one dword of the plane, sixteen bytes of the map).  `seams` counts the samples on the upper row of
 * the tile rows 1 .. and on the left column of the tile columns 1 ..: one lane each in the seam launch.  `chunks` counts the units of
 * HVQ_LB_LANES x 4 consecutive samples of the plane: a workgroup each in the launches that walk the map.  64 bytes. */
#define HVQ_LB_LANES 256u
#define HVQ_LB_TX    64u
#define HVQ_LB_TY    16u
#define HVQ_LB_TILE  (HVQ_LB_TX * HVQ_LB_TY)        /* 1024 samples: 4 KiB of parents in LDS */
#define HVQ_LB_CHUNK (HVQ_LB_LANES * 4u)            /* samples of a workgroup of the launches that walk the map */
#define HVQ_LB_SPAN  (HVQ_LB_LANES * 16u)           /* samples of one round of the numbering workgroup */
#define HVQ_LB_NUMBERED 0x80000000u                 /* a map entry that holds a component's number, not a parent */
typedef struct HvqLabelJob {
    uint64_t src;                      /* device address of the plane, a multiple of 4 */
    uint64_t labels;                   /* device address of uint32 [ny][nx], a multiple of 16 */
    uint64_t comps;                    /* device address of uint64 [cap + 1][8], a multiple of 16 */
    uint32_t nx, ny;                   /* the plane; nx is a multiple of 4, nx ny <= 2^26 */
    uint32_t tx, ty;                   /* tiles across and down */
    uint32_t seams;                    /* (ty - 1) nx + (tx - 1) ny */
    uint32_t chunks;                   /* ceil(nx ny / HVQ_LB_CHUNK) */
    uint32_t lo, hi;                   /* foreground: lo <= a <= hi */
    uint32_t conn;                     /* 4 or 8 */
    uint32_t cap;                      /* records the table has room for */
} HvqLabelJob;

/* one plane of one picture of the select launch (hvq_label.hip, hvq_select_components): three jobs a picture, Y, U, V, tiles and lanes
 * as in the map launch (HVQ_MP_*).  Y has body HVQ_SL_SELECT and reads `labels` and `comps`; U and V have HVQ_SL_FILL (128) and both 0.
 * 80 bytes. */
#define HVQ_SL_FILL   0u
#define HVQ_SL_SELECT 1u
typedef struct HvqSelectJob {
    uint64_t labels;                   /* device address of uint32 [dwords * 4], a multiple of 16 */
    uint64_t comps;                    /* device address of uint64 [cap + 1][8], a multiple of 16 */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    uint32_t dwords, tiles, body, cap;
    uint32_t area_min, area_max, w_min, w_max, h_min, h_max, invert;
    uint32_t pad[3];
} HvqSelectJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqLabelJob) == 64 && sizeof(HvqSelectJob) == 80, "job tables are uploaded in 16-byte units");
static_assert(HVQ_LB_TX * HVQ_LB_TY == HVQ_LB_LANES * 4u && HVQ_LB_TX % 4u == 0u, "a lane labels four samples of a tile row");
#else
_Static_assert(sizeof(HvqLabelJob) == 64 && sizeof(HvqSelectJob) == 80, "job tables are uploaded in 16-byte units");
#endif

/* one picture of the two distance launches (hvq_distance.hip, hvq_distance_pictures): the plane of the picture's rule and its distance
 * map, which is also the only working memory.  Grid row = picture in both launches.  Column pass: a workgroup of HVQ_DT_CLANES lanes owns
 * HVQ_DT_COLS consecutive columns, a lane four of them (one dword of the plane, sixteen bytes of the map a row).  Row pass: a workgroup of
 * HVQ_DT_LANES lanes owns `rows` whole rows, as many as fit HVQ_DT_SPAN samples of uint16 in LDS (16 KiB).  64 bytes. */
#define HVQ_DT_CLANES 64u
#define HVQ_DT_COLS   (HVQ_DT_CLANES * 4u)           /* columns of a workgroup of the column pass */
#define HVQ_DT_LANES  256u
#define HVQ_DT_SPAN   8192u                          /* samples of a workgroup of the row pass: the widest row there is */
#define HVQ_DT_INF    0xFFFFu                        /* a staged g of a column without background; the map holds 0xFFFFFFFF there */
typedef struct HvqDistanceJob {
    uint64_t src;                      /* device address of the plane, a multiple of 4 */
    uint64_t dist;                     /* device address of uint32 [ny][nx], a multiple of 16 */
    uint32_t nx, ny;                   /* the plane; nx is a multiple of 4 and at most HVQ_DT_SPAN */
    uint32_t lo, hi;                   /* foreground: lo <= a <= hi */
    uint32_t metric, border;           /* HVQ_DST_*; 0 or 1 */
    uint32_t colgroups;                /* ceil(nx / HVQ_DT_COLS) */
    uint32_t rows;                     /* min(ny, HVQ_DT_SPAN / nx) */
    uint32_t rowgroups;                /* ceil(ny / rows) */
    uint32_t pad[3];
} HvqDistanceJob;

/* one plane of one picture of the distance-mask launch (hvq_distance.hip, hvq_distance_mask): three jobs a picture, Y, U, V, tiles and
 * lanes as in the map launch (HVQ_MP_*).  Y has body HVQ_DM_RANGE or HVQ_DM_ROOT and reads `dist`; U and V have HVQ_DM_FILL (128).
 * 48 bytes. */
#define HVQ_DM_RANGE 0u                /* the modes of include/hvqm4_amd.h (HVQ_DSM_*) */
#define HVQ_DM_ROOT  1u
#define HVQ_DM_FILL  2u
typedef struct HvqDistMaskJob {
    uint64_t dist;                     /* device address of uint32 [dwords * 4], a multiple of 16 */
    uint64_t dst;                      /* device address of the target plane, a multiple of 4 */
    uint32_t dwords, tiles, body;
    uint32_t lo, hi, invert;
    uint32_t pad[2];
} HvqDistMaskJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqDistanceJob) == 64 && sizeof(HvqDistMaskJob) == 48, "job tables are uploaded in 16-byte units");
static_assert(HVQ_DT_SPAN % (HVQ_DT_LANES * 4u) == 0u, "a lane of the row pass takes four samples a round");
#else
_Static_assert(sizeof(HvqDistanceJob) == 64 && sizeof(HvqDistMaskJob) == 48, "job tables are uploaded in 16-byte units");
#endif

/* one picture of the two integral launches (hvq_integral.hip, hvq_integral_pictures): a plane and its inclusive summed-area tables, which
 * are also the only working memory.  Grid row = picture in both launches.  Row pass: a workgroup of HVQ_IG_RLANES lanes is HVQ_IG_WAVES
 * waves, a wave scans ONE row in chunks of HVQ_IG_CHUNK samples, a lane a dword of the plane a chunk.  Column pass: a workgroup of
 * HVQ_IG_CLANES lanes owns HVQ_IG_COLS consecutive columns, a lane four of them, and adds downwards.  48 bytes. */
#define HVQ_IG_WAVE   64u                            /* lanes of a wave: the width of the prefix */
#define HVQ_IG_WAVES  4u                             /* rows of a workgroup of the row pass */
#define HVQ_IG_RLANES (HVQ_IG_WAVE * HVQ_IG_WAVES)
#define HVQ_IG_CHUNK  (HVQ_IG_WAVE * 4u)             /* samples of a wave a step */
#define HVQ_IG_CLANES 64u
#define HVQ_IG_COLS   (HVQ_IG_CLANES * 4u)           /* columns of a workgroup of the column pass */
typedef struct HvqIntegralJob {
    uint64_t src;                      /* device address of the plane, a multiple of 4 */
    uint64_t sums;                     /* device address of uint32 [ny][nx], a multiple of 16 */
    uint64_t squares;                  /* device address of uint64 [ny][nx], a multiple of 16, or 0: no such table */
    uint32_t nx, ny;                   /* the plane; nx is a multiple of 4 */
    uint32_t rowgroups;                /* ceil(ny / HVQ_IG_WAVES) */
    uint32_t colgroups;                /* ceil(nx / HVQ_IG_COLS) */
    uint32_t chunks;                   /* ceil(nx / HVQ_IG_CHUNK) */
    uint32_t pad;
} HvqIntegralJob;

/* one picture of the window launch (hvq_integral.hip, hvq_window_pictures): the tables of a plane of Y's size, that plane, and the
 * picture written in slot layout.  Grid row = picture; a workgroup of HVQ_WN_LANES lanes takes a tile of HVQ_WN_TX x HVQ_WN_TY samples of
 * Y, a lane four adjacent samples (one dword stored), or, past the Y tiles, HVQ_WN_LANES * HVQ_WN_PER consecutive dwords of U | V, which
 * follow Y in a slot and are filled with 128.  80 bytes. */
#define HVQ_WN_TX     64u
#define HVQ_WN_TY     16u
#define HVQ_WN_LANES  256u
#define HVQ_WN_PER    8u                             /* chroma dwords of a lane */
#define HVQ_WN_MEAN      0u                          /* the modes of include/hvqm4_amd.h (HVQ_WIN_*) */
#define HVQ_WN_DEVIATION 1u
#define HVQ_WN_THRESHOLD 2u
#define HVQ_WN_MAX_AREA  (1u << 24)                  /* the samples of a window, of a rectangle: 255 * 2^24 < 2^32 */
typedef struct HvqWindowJob {
    uint64_t src;                      /* device address of the plane the tables are of (THRESHOLD reads it), a multiple of 4 */
    uint64_t sums;                     /* uint32 [ny][nx], a multiple of 16 */
    uint64_t squares;                  /* uint64 [ny][nx], a multiple of 16, or 0 where the rule needs none */
    uint64_t dst;                      /* device address of the picture written, a multiple of 16: Y, then cdwords dwords of 128 */
    uint32_t nx, ny;                   /* Y; nx is a multiple of 4 */
    uint32_t tx;                       /* ceil(nx / HVQ_WN_TX) */
    uint32_t ytiles;                   /* tx * ceil(ny / HVQ_WN_TY) */
    uint32_t cdwords;                  /* dwords of U | V */
    uint32_t tiles;                    /* ytiles + ceil(cdwords / (HVQ_WN_LANES * HVQ_WN_PER)) */
    uint32_t mode, rx, ry;
    int32_t k, c;
    uint32_t invert;
} HvqWindowJob;

/* the rectangle launch (hvq_integral.hip, hvq_rect_sums): ONE head, then one HvqRectTables a picture.  A lane a rectangle. */
#define HVQ_RC_LANES 256u
typedef struct HvqRectHead {
    uint64_t rects;                    /* device address of int32 [nrects][5]: i, x0, y0, x1, y1 */
    uint64_t dims;                     /* device address of uint32 [npics][2]: nx, ny */
    uint64_t out;                      /* device address of uint64 [nrects][3]: count, S, Q */
    uint32_t nrects, npics;
} HvqRectHead;
typedef struct HvqRectTables { uint64_t sums, squares; } HvqRectTables;      /* of picture i; squares 0: Q comes out 0 */

#if defined(__cplusplus)
static_assert(sizeof(HvqIntegralJob) == 48 && sizeof(HvqWindowJob) == 80 && sizeof(HvqRectHead) == 32 && sizeof(HvqRectTables) == 16, "job tables are uploaded in 16-byte units");
static_assert(HVQ_WN_TX * HVQ_WN_TY == HVQ_WN_LANES * 4u && HVQ_WN_TX % 4u == 0u, "a lane of the window launch takes four adjacent samples");
#else
_Static_assert(sizeof(HvqIntegralJob) == 48 && sizeof(HvqWindowJob) == 80 && sizeof(HvqRectHead) == 32 && sizeof(HvqRectTables) == 16, "job tables are uploaded in 16-byte units");
#endif

/* one picture of the four corner launches (hvq_corner.hip, hvq_corner_pictures): the plane of the picture's rule, the same plane of the
 * mask picture, the two planes of the mask that are only filled, and the lists.  Grid row = picture in every launch.  A tile is
 * HVQ_CR_TX x HVQ_CR_TY targets; a workgroup of HVQ_CR_LANES lanes stages its bytes with a halo of nms + radius + 1 rows and
 * HVQ_CR_HX columns (whole dwords), a lane stores one dword of the mask.  The workgroups of a grid row of launch 1 walk the tx ty tiles
 * of the analysed plane, then the fill tiles (HVQ_CR_FILL dwords each) of the two other planes; those past them leave.  In LDS
 * (hvq_corner.h says what lies where): the staged bytes and the packed gradients, over which the responses are written later, and the
 * three horizontal sums.  Every member is a dword or a qword; 128 bytes. */
#define HVQ_CR_LANES   256u
#define HVQ_CR_TX      64u
#define HVQ_CR_TY      16u
#define HVQ_CR_MAX_R   3u            /* HVQ_CRN_MAX_RADIUS */
#define HVQ_CR_MAX_NMS 7u            /* HVQ_CRN_MAX_NMS */
#define HVQ_CR_HX      12u           /* bytes staged left and right of a tile's 64: nms + radius + 1 <= 11 rounded up to whole dwords */
#define HVQ_CR_SD      ((HVQ_CR_TX + 2u * HVQ_CR_HX) / 4u)                              /* 22 dwords a staged row */
#define HVQ_CR_SROWS   (HVQ_CR_TY + 2u * (HVQ_CR_MAX_NMS + HVQ_CR_MAX_R + 1u))         /* 38 staged rows at the most */
#define HVQ_CR_GROWS   (HVQ_CR_TY + 2u * (HVQ_CR_MAX_NMS + HVQ_CR_MAX_R))              /* 36 rows of gradients */
#define HVQ_CR_GS      85u           /* dwords a row of gradients: 64 + 2 (7 + 3) = 84 and one more, an odd pitch for the lanes that walk rows */
#define HVQ_CR_HS      79u           /* dwords a row of horizontal sums and qwords a row of responses: 64 + 2 7 = 78 and one more */
#define HVQ_CR_RROWS   (HVQ_CR_TY + 2u * HVQ_CR_MAX_NMS)                               /* 30 rows of responses */
#define HVQ_CR_S_AT    0u
#define HVQ_CR_G_AT    (HVQ_CR_SROWS * HVQ_CR_SD)                                        /* 836 */
#define HVQ_CR_R_AT    0u            /* the responses lie over the staged bytes and the gradients, which are dead by then */
#define HVQ_CR_H_AT    (2u * HVQ_CR_RROWS * HVQ_CR_HS)                                   /* 4740 */
#define HVQ_CR_HPLANE  (HVQ_CR_GROWS * HVQ_CR_HS)                                        /* 2844 dwords each of the sums of gx gx, gx gy, gy gy */
#define HVQ_CR_LDS     (HVQ_CR_H_AT + 3u * HVQ_CR_HPLANE)                                /* 13272 dwords: 53088 bytes, three workgroups a CU */
#define HVQ_CR_HSEG    13u           /* columns a lane of the horizontal pass slides along: 36 rows x 6 segments <= 256 lanes */
#define HVQ_CR_VSEG    10u           /* rows a lane of the vertical pass slides down: 78 columns x 3 segments <= 256 lanes */
#define HVQ_CR_FILL    (HVQ_CR_LANES * 4u)   /* dwords of a fill tile: sixteen bytes a lane */
typedef struct HvqCornerJob {
    uint64_t src;                      /* device address of the analysed plane, a multiple of 4 */
    uint64_t mask;                     /* device address of the same plane of the mask picture, a multiple of 4 */
    uint64_t points;                   /* device address of int64 [cap + 1][4], a multiple of 16 */
    uint64_t rows;                     /* device address of uint32 [ny + 1], a multiple of 16 */
    uint64_t response;                 /* device address of int64 [ny][nx], a multiple of 16; 0: none */
    uint64_t fill[2];                  /* device addresses of the two other planes of the mask picture, multiples of 4 */
    int64_t threshold;
    uint32_t nx, ny;                   /* the plane; nx is a multiple of 4 */
    uint32_t tx, ty;                   /* tiles across and down */
    uint32_t mode, radius, k, nms, margin;
    uint32_t cap;                      /* rows the list has room for */
    uint32_t fill_dwords[2], fill_value[2], fill_tiles[2];
} HvqCornerJob;

#if defined(__cplusplus)
static_assert(sizeof(HvqCornerJob) == 128, "job tables are uploaded in 16-byte units");
static_assert(HVQ_CR_TX * HVQ_CR_TY == HVQ_CR_LANES * 4u && HVQ_CR_TX == 64u, "a lane stores one dword of the tile");
static_assert(HVQ_CR_HX >= HVQ_CR_MAX_NMS + HVQ_CR_MAX_R + 1u && HVQ_CR_HX % 4u == 0u, "the staged row: whole dwords that hold the halo");
static_assert(HVQ_CR_GS > HVQ_CR_TX + 2u * (HVQ_CR_MAX_NMS + HVQ_CR_MAX_R) && HVQ_CR_HS > HVQ_CR_TX + 2u * HVQ_CR_MAX_NMS, "the pitches hold the widest rows");
static_assert(HVQ_CR_G_AT + HVQ_CR_GROWS * HVQ_CR_GS <= HVQ_CR_H_AT && HVQ_CR_R_AT % 2u == 0u, "the responses cover the staged bytes and the gradients, as qwords");
static_assert(HVQ_CR_GROWS * ((HVQ_CR_TX + 2u * HVQ_CR_MAX_NMS + HVQ_CR_HSEG - 1u) / HVQ_CR_HSEG) <= HVQ_CR_LANES, "a lane a segment of the horizontal pass");
static_assert((HVQ_CR_TX + 2u * HVQ_CR_MAX_NMS) * ((HVQ_CR_RROWS + HVQ_CR_VSEG - 1u) / HVQ_CR_VSEG) <= HVQ_CR_LANES, "a lane a segment of the vertical pass");
#else
_Static_assert(sizeof(HvqCornerJob) == 128, "job tables are uploaded in 16-byte units");
#endif


#endif
