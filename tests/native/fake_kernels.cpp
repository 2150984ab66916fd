/*
 * tests/native/fake_kernels.cpp -- TEST INFRASTRUCTURE: CPU bodies for the hvq_launch_* entry points and the LDS / occupancy helpers that
 * hvqm4_amd/csrc/hvq_runtime.cpp imports from the HIP units, for the CPU fake device (fake_device.cpp).  A launch is queued on its stream
 * like any other operation and its body runs when the scheduler says so; every body reaches memory only through fake_span, at that moment.
 *
 * Reconstruction is NOT restated here: the launch walks its grid the way hvq_recon_inline_kernel does (job slots x workgroups, the
 * kernel's plane and tile mapping) and hands every tile a workgroup covers to the scalar descriptor interpreter (oracle/hvq_desc_recon.c,
 * front end 2: the view of an HvqJob record).  Before that it asserts what the GPU would silently get wrong (a short items_cap, a staged
 * pool that is no multiple of 4 dwords) and the footprints of the kernel's wide loads, each with the kernel line it restates.  Lanes, LDS
 * and barriers are not emulated.  The colour and filter kernels do no arithmetic (the bit-exact GPU tests own that): they check their
 * sources, tables and destination rows, log a hash of the source planes as read when they run, and fill the destination with a marker.
 * The LDS and scratch sizing helpers the runtime imports are restated in fake_helpers.cpp.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/hvqm4_amd.h"
#include "../../oracle/hvq_desc_recon.h"
#include "../../hvqm4_amd/csrc/hvq_gparse_core.h"

extern "C" int gparse_emul_job(const HvqParseJob *job, HvqParseResult *res, int mode);       /* gparse_emul.c */

static std::vector<FakeExportRecord> g_log;
static int g_export_calls = 0;
const std::vector<FakeExportRecord> &fake_export_log(void) { return g_log; }

template <class T> static const T *span_of(uint64_t addr, size_t count, const char *what)
{
    return (const T *)fake_span((const void *)(uintptr_t)addr, count * sizeof(T), what);
}

/* ------------------------------------------------------------------ reconstruction */
static void view_of_job(const HvqJob &J, HvqdView *v)
{
    memset(v, 0, sizeof *v);
    const bool is_pb = ((J.flags >> HVQ_JOB_KIND_SHIFT) & 3u) != HVQ_PIC_I;
    v->flags = J.flags & 0xFFFFu;
    v->pic_kind = (J.flags >> HVQ_JOB_KIND_SHIFT) & 3u;
    v->unk_shift = (J.flags >> HVQ_JOB_UNK_SHIFT) & 31u;
    v->width = J.width; v->mcb_w = J.mcb_w;
    v->slot_bytes = J.slot_bytes; v->total_tiles = J.total_tiles;
    for (int k = 0; k < 3; ++k) {
        HvqdPlane &P = v->pl[k];
        const HvqPlaneRec &r = J.plane[k];
        P.hb = (int)(r.hbvb & 0xFFFFu); P.vb = (int)(r.hbvb >> 16);
        P.pw = (int)(r.pw_sub & 0xFFFFu); P.ws = (int)((r.pw_sub >> 16) & 0xFFu); P.hs = (int)(r.pw_sub >> 24);
        P.plane_off = r.plane_off; P.tile_first = r.tile_first;
        P.map = span_of<uint8_t>(r.map, (size_t)(P.hb + 2) * (size_t)(P.vb + 2) * 2u, "recon: a plane's map");
        P.dst = (uint8_t *)span_of<uint8_t>(r.dst, (size_t)P.pw * (size_t)P.vb * 4u, "recon: a plane of the destination picture");
    }
    v->mcb_h = (uint32_t)v->pl[0].vb / 2u;                                       /* hvq_selfref_kernel: (hbvb >> 16) / 2 */
    v->pool = (const uint32_t *)(uintptr_t)J.pool;                               /* checked range by range below */
    v->wave_base = span_of<uint32_t>(J.wave_base, (size_t)J.total_tiles * (HVQ_TILE_BLOCKS / 64), "recon: wave_base");
    if (is_pb) {
        v->mvs = (const int16_t *)span_of<uint32_t>(J.mv, (size_t)J.mcb_w * v->mcb_h, "recon: macroblock vectors");
        v->ref0 = span_of<uint8_t>(J.ring + J.ref0_off, J.slot_bytes, "recon: the past picture's slot");
        v->ref1 = span_of<uint8_t>(J.ring + J.ref1_off, J.slot_bytes, "recon: the future picture's slot");
    }
    /* hvq_kernels.hip:763-769: the nest goes to LDS in HVQ_NESTP_BYTES / 16 = 84 pieces of 16 bytes */
    hvqd_view_set_nest(v, J.nest ? span_of<uint8_t>(J.nest, 84u * 16u, "recon: the 84 nest pieces") : nullptr);
    if (J.q_offs_off)
        v->q_offs = (uint32_t *)span_of<uint32_t>(J.tq + J.q_offs_off, (size_t)J.total_tiles * HVQ_TILE_BLOCKS, "recon: the blocks' pool offsets for the raster walk");
}

static inline int clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

/* what one workgroup loads with wide loads for tile `tile` (of the plane) -- none of it may leave its allocation */
static void tile_footprints(const HvqJob &J, const HvqdView &v, int p, uint32_t tile)
{
    const HvqdPlane &P = v.pl[p];
    const bool is_pb = v.pic_kind != HVQ_PIC_I, is15 = v.flags & HVQ_F_IS15;
    const uint32_t nblocks = (uint32_t)P.hb * (uint32_t)P.vb, stride = (uint32_t)P.hb + 2u;
    for (uint32_t t = 0; t < HVQ_TILE_BLOCKS; ++t) {
        const uint32_t b = tile * HVQ_TILE_BLOCKS + t;
        if (b >= nblocks) break;
        const uint32_t by = b / (uint32_t)P.hb, bx = b % (uint32_t)P.hb;
        const uint8_t *own = P.map + 2u * ((size_t)(by + 1u) * stride + bx + 1u);
        /* hvq_kernels.hip:749: row8 = one 8-byte load at the entry to the left: left, own, right and one more entry */
        fake_span(own - 2, 8, "recon: the 8-byte map load of the left, own and right entries");
        /* hvq_kernels.hip:753: the two vertical neighbours, 2 bytes each */
        fake_span(own - 2u * stride, 2, "recon: the map entry above");
        fake_span(own + 2u * stride, 2, "recon: the map entry below");
        if (!is_pb) continue;
        const uint32_t T = own[1], kind = T & 0xFu;
        const bool inter = T & 0x60u, proc = T & 0x10u;
        if (!(inter && (proc || kind != 6u))) continue;                          /* inl_classify: mc */
        /* hvq_kernels.hip:756: the macroblock's vector */
        const uint32_t mvw = *span_of<uint32_t>(J.mv + 4u * ((size_t)(by >> (1 - P.hs)) * J.mcb_w + (bx >> (1 - P.ws))), 1, "recon: a macroblock vector");
        const int rx = (int16_t)(mvw & 0xFFFFu), ry = (int32_t)mvw >> 16;
        const int hsy = is15 ? P.hs : 0;
        const bool hy = (ry >> hsy) & 1;
        /* hvq_kernels.hip:822-828: the block's source address, clamped once for all its rows */
        const int rowi = (ry >> (P.hs + 1)) + (int)((by & (uint32_t)(1 - P.hs)) << 2);
        const int coli = (rx >> (P.ws + 1)) + (int)((bx & (uint32_t)(1 - P.ws)) << 2) + (int)P.plane_off;
        const int hi3 = (int)J.slot_bytes - 8 - 3 * P.pw, hi4 = hi3 - P.pw;
        const int a = clampi(rowi * P.pw + coli, 0, hy ? hi4 : hi3);
        const uint32_t roff = (T & 0x60u) == 0x20u ? J.ref0_off : J.ref1_off;
        /* hvq_kernels.hip:846-848: four 8-byte rows, five with a vertical half sample */
        for (int y = 0; y < (hy ? 5 : 4); ++y)
            span_of<uint8_t>(J.ring + (uint32_t)(roff + (uint32_t)a + (uint32_t)y * (uint32_t)P.pw), 8, "recon: an 8-byte motion-compensation row");
    }
}

static uint32_t fullest_tile_items(const HvqdView &v)
{
    const bool is_pb = v.pic_kind != HVQ_PIC_I;
    uint32_t best = 0;
    for (int p = 0; p < 3; ++p) {
        const HvqdPlane &P = v.pl[p];
        const uint32_t nblocks = (uint32_t)P.hb * (uint32_t)P.vb;
        for (uint32_t b0 = 0; b0 < nblocks; b0 += HVQ_TILE_BLOCKS) {
            uint32_t items = 0;
            for (uint32_t b = b0; b < std::min(nblocks, b0 + HVQ_TILE_BLOCKS); ++b) {
                const uint32_t T = P.map[2u * ((size_t)(b / (uint32_t)P.hb + 1u) * ((uint32_t)P.hb + 2u) + b % (uint32_t)P.hb + 1u) + 1u];
                const uint32_t kind = (!is_pb && p == 0) ? T : (T & 0xFu);
                const bool k068 = kind == 0u || kind == 6u || kind == 8u;
                const bool inter = is_pb && (T & 0x60u), proc = T & 0x10u;
                /* inl_classify: class 1 (intra AOT) and class 2 (MC-residual) blocks are the items */
                if (inter ? (!proc && kind != 0u && kind != 6u) : !k068) ++items;
            }
            best = std::max(best, items);
        }
    }
    return best;
}

extern "C" hipError_t hvq_launch_recon_inline(const HvqJob *jobs_dev, uint32_t nslots, uint32_t max_wgs, uint32_t tiles_per_wg,
                                              uint32_t items_cap, uint32_t pair_cap, uint32_t pool_cap, hipStream_t stream)
{
    if (nslots == 0 || max_wgs == 0) return hipSuccess;
    /* the staged pool is filled in 16-byte pieces (hvq_launch_recon_inline rounds a ragged size up, and the host's LDS sum would be short) */
    if (pool_cap & 3u) fake_die("recon launch: pool_cap %u is not a multiple of 4 dwords", pool_cap);
    if (tiles_per_wg != 1 && tiles_per_wg != 2) fake_die("recon launch: %u tiles per workgroup", tiles_per_wg);
    (void)pair_cap;                                                              /* a short pair list turns a tile serial: slower, not wrong */
    return fake_enqueue(stream, "recon", [=]() {
        const uint32_t TPW = tiles_per_wg;
        fake_span(jobs_dev, (size_t)nslots * sizeof(HvqJob), "recon: the launch's job records");
        HvqdView *v = new HvqdView;
        for (uint32_t s = 0; s < nslots; ++s) {
            const HvqJob &J = jobs_dev[s];
            if (J.total_tiles == 0) continue;                                    /* padding slot or dropped picture: its workgroups exit */
            view_of_job(J, v);
            /* inline_sized (hvq_runtime.cpp): "items beyond the cap are dropped" */
            const uint32_t fullest = fullest_tile_items(*v), need = std::min(256u * TPW, TPW * fullest);
            if (items_cap < need) fake_die("recon launch: items_cap %u below %u (%u tile(s) per workgroup, fullest tile %u items): the kernel drops the rest", items_cap, need, TPW, fullest);
            /* hvq_kernels.hip:625-628: the workgroup's plane from the first tiles beside the common part of the record */
            const uint32_t n0 = J.tile_first12[0], n1 = J.tile_first12[1] - J.tile_first12[0], n2 = J.total_tiles - J.tile_first12[1];
            const uint32_t pf1 = (n0 + TPW - 1) / TPW, pf2 = pf1 + (n1 + TPW - 1) / TPW, pend = pf2 + (n2 + TPW - 1) / TPW;
            for (uint32_t wg = 0; wg < max_wgs; ++wg) {
                if (wg >= pend) break;
                const int p = (wg >= pf1) + (wg >= pf2);
                const uint32_t nplane_tiles = p == 0 ? n0 : p == 1 ? n1 : n2;
                const uint32_t pairw = wg - (p == 0 ? 0u : p == 1 ? pf1 : pf2);
                const uint32_t tile0 = v->pl[p].tile_first + TPW * pairw;         /* hvq_kernels.hip:667 */
                const uint32_t ntl = std::min(TPW, nplane_tiles - TPW * pairw);
                /* hvq_kernels.hip:709-713: wave_base of the workgroup's tiles, and of the tile behind them */
                span_of<uint32_t>(J.wave_base + 4u * (size_t)tile0 * (HVQ_TILE_BLOCKS / 64), (size_t)ntl * (HVQ_TILE_BLOCKS / 64), "recon: the wave_base dwords of a workgroup");
                const uint32_t plo = v->wave_base[tile0 * (HVQ_TILE_BLOCKS / 64)];
                uint32_t phi = tile0 + ntl < J.total_tiles ? v->wave_base[(tile0 + ntl) * (HVQ_TILE_BLOCKS / 64)] : J.pool_dwords;
                /* hvq_kernels.hip:771-778: the tile range of the pool, from the 16-byte boundary below its first dword, in 16-byte pieces */
                phi = std::max(phi, plo);
                const uint32_t plo4 = plo & ~3u, nst = std::min(phi - plo4, pool_cap), nch = (nst + 3u) >> 2;
                if (nch) span_of<uint8_t>(J.pool + 4u * (size_t)plo4, 16u * (size_t)nch, "recon: the staged pool range of a workgroup");
                if (phi > J.pool_dwords) fake_die("recon: a tile's payload ends at dword %u of a pool of %u", phi, J.pool_dwords);
                if (phi > plo) span_of<uint32_t>(J.pool + 4u * (size_t)plo, phi - plo, "recon: the payload of a workgroup's tiles");
                for (uint32_t h = 0; h < ntl; ++h) {
                    tile_footprints(J, *v, p, TPW * pairw + h);
                    hvqd_view_tile(v, p, TPW * pairw + h);
                }
            }
        }
        delete v;
    });
}

extern "C" hipError_t hvq_launch_selfref(const HvqJob *job_dev, const uint8_t *side, uint8_t *dst, hipStream_t stream)
{
    return fake_enqueue(stream, "selfref", [=]() {
        fake_span(job_dev, sizeof(HvqJob), "selfref: the job record");
        const HvqJob &J = *job_dev;
        if (!J.q_offs_off) fake_die("selfref: the picture's job has no section of pool offsets");
        HvqdView *v = new HvqdView;
        view_of_job(J, v);
        const size_t pic_bytes = (size_t)v->pl[2].plane_off + (size_t)v->pl[2].pw * (size_t)v->pl[2].vb * 4u;
        fake_span(side, pic_bytes, "selfref: the side buffer");
        fake_span(dst, J.slot_bytes, "selfref: the picture's slot");
        if (J.pool_dwords) span_of<uint32_t>(J.pool, J.pool_dwords, "selfref: the pool");
        hvqd_view_selfref(v, side, dst);
        delete v;
    });
}

/* ------------------------------------------------------------------ small kernels, restated */
extern "C" hipError_t hvq_launch_upload(const void *src_pinned, void *dst_dev, size_t bytes, hipStream_t stream)
{
    const size_t n16 = (bytes + 15u) / 16u;                                      /* hvq_upload_kernel moves whole 16-byte units: the padding too */
    if (!n16) return hipSuccess;
    if (((uintptr_t)src_pinned | (uintptr_t)dst_dev) & 15u) fake_die("upload: source or destination is not 16-byte aligned");
    return fake_enqueue(stream, "upload", [=]() {
        fake_span(src_pinned, n16 * 16u, "upload: the pinned source, padding included");
        fake_span(dst_dev, n16 * 16u, "upload: the destination, padding included");
        memcpy(dst_dev, src_pinned, n16 * 16u);                                  /* the source is read NOW */
    });
}

extern "C" hipError_t hvq_launch_nest_commit(const uint64_t *pairs_dev, uint32_t n, hipStream_t stream)
{
    if (!n) return hipSuccess;
    return fake_enqueue(stream, "nest commit", [=]() {
        fake_span(pairs_dev, (size_t)n * 16u, "nest commit: the pairs");
        for (uint32_t k = 0; k < n; ++k)
            memcpy((void *)span_of<uint8_t>(pairs_dev[2 * k + 1], GP_ALIGN16(HVQ_NESTP_BYTES), "nest commit: a kept nest"),
                   span_of<uint8_t>(pairs_dev[2 * k], GP_ALIGN16(HVQ_NESTP_BYTES), "nest commit: a batch's nest"), GP_ALIGN16(HVQ_NESTP_BYTES));
    });
}

extern "C" hipError_t hvq_launch_gather(const uint64_t *src_dev, uint8_t *dst_dev, uint32_t n, uint32_t pic_bytes, hipStream_t stream)
{
    if (!n) return hipSuccess;
    if (pic_bytes & 15u) fake_die("gather: %u bytes per picture: hvq_gather_kernel moves 16-byte units and would drop the tail", pic_bytes);
    return fake_enqueue(stream, "gather", [=]() {
        fake_span(src_dev, (size_t)n * 8u, "gather: the slot addresses");
        for (uint32_t i = 0; i < n; ++i)
            memcpy((void *)fake_span(dst_dev + (size_t)i * pic_bytes, pic_bytes, "gather: the staging buffer"), span_of<uint8_t>(src_dev[i], pic_bytes, "gather: a picture's slot"), pic_bytes);
    });
}

extern "C" hipError_t hvq_launch_table_div(uint32_t *out_dev, hipStream_t stream)
{
    return fake_enqueue(stream, "table div", [=]() {
        fake_span(out_dev, 272u * 4u, "table div: the output");
        for (uint32_t d = 0; d < 16u; ++d) out_dev[d] = d ? 256u / d : 0u;
        for (uint32_t d = 0; d < 256u; ++d) out_dev[16u + d] = d ? 4096u / d : 0u;
    });
}

/* ------------------------------------------------------------------ the parse kernel: the GPU parse core, thread by thread (gparse_emul.c) */
extern "C" hipError_t hvq_launch_parse(const HvqParseJob *jobs_dev, HvqParseResult *results_dev, uint32_t n, uint32_t rowbuf_stride, uint32_t use_flat,
                                       const uint32_t *redo_dev, uint64_t *, hipStream_t stream)
{
    if (!n) return hipSuccess;
    return fake_enqueue(stream, "parse", [=]() {
        if (redo_dev) fake_span(redo_dev, (size_t)n * 4u, "parse: the redo list");
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t pic = redo_dev ? redo_dev[k] : k;                     /* hvq_gparse.hip:852 */
            const HvqParseJob job = *(const HvqParseJob *)fake_span(jobs_dev + pic, sizeof(HvqParseJob), "parse: a job record");
            HvqParseResult *res = (HvqParseResult *)fake_span(results_dev + pic, sizeof(HvqParseResult), "parse: a result record");
            uint32_t blocks = 0, runs = 0;
            for (int i = 0; i < 3; ++i) {
                const int ws = i ? job.h_samp == 2 : 0, hs = i ? job.v_samp == 2 : 0;
                const uint32_t nb = (uint32_t)((job.width >> ws) / 4) * (uint32_t)((job.height >> hs) / 4);
                blocks += nb; runs += (nb + HVQ_TILE_BLOCKS - 1) / HVQ_TILE_BLOCKS * (HVQ_TILE_BLOCKS / 64);
            }
            span_of<uint8_t>(job.pic, (size_t)job.pic_dwords * 4u, "parse: the bitstream with its zero padding");
            if ((size_t)job.pic_dwords * 4u < (size_t)job.len) fake_die("parse: %u dwords for a picture of %u bytes", job.pic_dwords, job.len);
            span_of<uint8_t>(job.blob, job.cap, "parse: the blob");
            span_of<uint8_t>(job.scratch, gp_scratch_bytes(blocks, runs, (uint32_t)(job.width / 8) * (uint32_t)(job.height / 8)), "parse: the scratch");
            if (job.frame_type == HVQ_FRAME_I) span_of<uint8_t>(job.nest_out, GP_ALIGN16(HVQ_NESTP_BYTES), "parse: the nest of an I picture");
            /* hvq_gparse.hip:904: the DC row buffers in LDS are as wide as the host said */
            if ((uint32_t)(job.width / 4 + 2) > rowbuf_stride) fake_die("parse: rowbuf_stride %u below the %u entries of a luma row", rowbuf_stride, job.width / 4 + 2);
            HvqParseResult r;
            memset(&r, 0, sizeof r);
            /* FLAT kernel: a picture it cannot serve goes back marked 2 (hvq_gparse.hip:1108); the chains serve every picture */
            const int rc = gparse_emul_job(&job, &r, use_flat ? 2 : 0);
            if (rc < 0) fake_die("parse: out of memory");
            if (rc == 1) { memset(&r, 0, sizeof r); r.pad[0] = 2u; }
            else r.pad[0] = 0u;
            *res = r;
        }
    });
}

/* ------------------------------------------------------------------ colour and filter kernels: footprints, a log, a marker */
static uint64_t fnv1a(const uint8_t *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

/* the source planes Y | U | V of a slot as the records describe them (U starts where Y ends, V where U ends), hashed as read now */
static void log_source(int call, int job, const uint8_t *y, const uint8_t *u, const uint8_t *v)
{
    if (!(y < u && u < v)) fake_die("export: the source planes of job %d are not Y | U | V", job);
    const size_t ny = (size_t)(u - y), nc = (size_t)(v - u);
    fake_span(y, ny + 2 * nc, "export: the source planes of a picture");
    g_log.push_back(FakeExportRecord{ call, job, fnv1a(y, ny + 2 * nc) });
}

static void mark_rows(uint8_t *dst, int planes, int rows, size_t row_bytes, int64_t row_pitch, int64_t plane_pitch, const char *what)
{
    for (int c = 0; c < planes; ++c)
        for (int i = 0; i < rows; ++i) {
            uint8_t *row = dst + (int64_t)c * plane_pitch + (int64_t)i * row_pitch;
            memset((void *)fake_span(row, row_bytes, what), 0xEE, row_bytes);
        }
}

extern "C" hipError_t hvq_launch_rgb(const void *jobs_dev, int njobs, int, int, int format, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    if (format != HVQ_FMT_RGB24 && format != HVQ_FMT_RGBP && format != HVQ_FMT_YUV444P) return hipErrorInvalidValue;
    const int call = g_export_calls++;
    return fake_enqueue(stream, "rgb", [=]() {
        const HvqRgbJob *j = (const HvqRgbJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqRgbJob), "rgb: the job records");
        for (int k = 0; k < njobs; ++k) {
            if ((size_t)(j[k].u - j[k].y) != (size_t)j[k].w * (size_t)j[k].h) fake_die("rgb: job %d: the luma plane is not w x h", k);
            log_source(call, k, j[k].y, j[k].u, j[k].v);
            if (format == HVQ_FMT_RGB24) mark_rows(j[k].dst, 1, j[k].h, (size_t)j[k].w * 3u, j[k].row_pitch, 0, "rgb: a destination row");
            else mark_rows(j[k].dst, 3, j[k].h, (size_t)j[k].w, j[k].row_pitch, j[k].plane_pitch, "rgb: a destination row");
        }
    });
}

extern "C" hipError_t hvq_launch_tensor(const void *jobs_dev, int njobs, int, int dtype, const HvqTensorNorm *, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    const size_t es = dtype == HVQ_T_F32 ? 4 : 2;
    const int call = g_export_calls++;
    return fake_enqueue(stream, "tensor", [=]() {
        const HvqTensorJob *j = (const HvqTensorJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqTensorJob), "tensor: the job records");
        for (int k = 0; k < njobs; ++k) {
            if ((size_t)(j[k].u - j[k].y) != (size_t)j[k].w * (size_t)j[k].h) fake_die("tensor: job %d: the luma plane is not w x h", k);
            if (j[k].x0 < 0 || j[k].y0 < 0 || j[k].x0 + j[k].cw > j[k].w || j[k].y0 + j[k].ch > j[k].h) fake_die("tensor: job %d: the crop leaves the picture", k);
            log_source(call, k, j[k].y, j[k].u, j[k].v);
            mark_rows(j[k].dst, 3, j[k].out_h, (size_t)j[k].out_w * es, j[k].row_pitch, j[k].plane_pitch, "tensor: a destination row");
        }
    });
}

extern "C" hipError_t hvq_launch_resample(const void *jobs_dev, int njobs, int, int dtype, const HvqTensorNorm *, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    const size_t es = dtype == HVQ_T_F32 ? 4 : 2;
    const int call = g_export_calls++;
    return fake_enqueue(stream, "resample", [=]() {
        const HvqResampleJob *j = (const HvqResampleJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqResampleJob), "resample: the job records");
        const uint8_t *tabs = (const uint8_t *)(j + njobs);                      /* hvq_launch_resample: the tables lie behind the records */
        for (int k = 0; k < njobs; ++k) {
            const int h = (int)((size_t)(j[k].u - j[k].y) / (size_t)j[k].w);
            /* one axis: int32 first[n], int32 start[n + 1], float w[start[n]]; every tap stays inside the picture */
            auto axis = [&](uint32_t off, int n_out, int origin, int limit, const char *what) {
                const int32_t *first = (const int32_t *)fake_span(tabs + off, (size_t)(2 * n_out + 1) * 4u, what);
                const int32_t *start = first + n_out;
                fake_span(start + n_out + 1, (size_t)start[n_out] * 4u, what);
                for (int o = 0; o < n_out; ++o)
                    if (first[o] < 0 || start[o + 1] <= start[o] || origin + first[o] + (start[o + 1] - start[o]) > limit) fake_die("%s: output %d reads outside the picture", what, o);
            };
            axis(j[k].xtab, j[k].out_w, j[k].x0, j[k].w, "resample: the column table");
            axis(j[k].ytab, j[k].out_h, j[k].y0, h, "resample: the row table");
            log_source(call, k, j[k].y, j[k].u, j[k].v);
            mark_rows(j[k].dst, 3, j[k].out_h, (size_t)j[k].out_w * es, j[k].row_pitch, j[k].plane_pitch, "resample: a destination row");
        }
    });
}
