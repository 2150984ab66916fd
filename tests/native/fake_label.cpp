/*
 * tests/native/fake_label.cpp -- TEST INFRASTRUCTURE: the CPU bodies of hvq_launch_label and hvq_launch_select (hvqm4_amd/csrc/hvq_label.hip)
 * for the CPU fake device.  Linked into the label driver only (tests/test_label_cpu.py); the other drivers link without it, and the
 * runtime's weak references then make hvq_label_pictures and hvq_select_components refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grids of the launches the way the kernels
 * do, lane by lane, with the functions of hvq_label.h, whose atomic steps are plain ones here (HVQ_LB_PLAIN: one lane runs at a time).
 *   label:   every job record is checked against hvq_lb_job, and the plane, the map and the record table must each lie inside one live
 *            allocation (fake_span) before a lane touches them.  Then the seven launches one behind the other: begin; the tiles, each over
 *            an array of the kernel's LDS size on the heap filled with a pattern (the sanitised build sees an index outside it); the
 *            seam items; flatten; the numbering rounds with the workgroup's scan; resolve, every lane flushing its own last run; finish.  The
 *            tile launch must store every element of the map exactly once: the map is filled with a pattern no tile stores, and a
 *            count of the tiles' lanes per element is kept.  After the last launch no entry may carry the mark, and no entry may exceed K.
 *   select:  planes x tiles x lanes as in the map launch; every target dword must be stored exactly once.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HVQ_LB_PLAIN 1
#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_map.h"
#include "../../hvqm4_amd/csrc/hvq_label.h"

#define EACH_LANE(n) for (uint32_t lane = 0; lane < (n); ++lane)

static void label_picture(int k, const HvqLabelJob &J, uint32_t max_tiles, uint32_t max_seams, uint32_t max_chunks)
{
    if (!J.nx || !J.ny || (J.nx & 3u) || (uint64_t)J.nx * J.ny > (1u << 26) || (J.src & 3u) || !J.labels || (J.labels & 15u) || !J.comps || (J.comps & 15u))
        fake_die("label: job %d: a plane of %u x %u at %#llx, the map at %#llx, the records at %#llx", k, J.nx, J.ny, (unsigned long long)J.src,
                 (unsigned long long)J.labels, (unsigned long long)J.comps);
    if (J.lo > J.hi || J.hi > 255u || (J.conn != 4u && J.conn != 8u) || J.cap > (1u << 20)) fake_die("label: job %d: window %u .. %u, connectivity %u, cap %u", k, J.lo, J.hi, J.conn, J.cap);
    const HvqLabelJob A = hvq_lb_job(J.src, J.labels, J.comps, J.nx, J.ny, J.lo, J.hi, J.conn, J.cap);
    if (memcmp(&A, &J, sizeof J)) fake_die("label: job %d: the record is not hvq_lb_job's for %u x %u", k, J.nx, J.ny);
    if (J.tx * J.ty > max_tiles || J.seams > max_seams || J.chunks > max_chunks)
        fake_die("label: job %d needs %u tiles, %u seam items, %u chunks; the grids have %u, %u, %u", k, J.tx * J.ty, J.seams, J.chunks, max_tiles, max_seams, max_chunks);
    const uint32_t N = J.nx * J.ny;
    fake_span((const void *)(uintptr_t)J.src, N, "label: the plane");
    uint32_t *L = (uint32_t *)fake_span((const void *)(uintptr_t)J.labels, 4u * (size_t)N, "label: the map");
    uint64_t *C = (uint64_t *)fake_span((const void *)(uintptr_t)J.comps, 64u * ((size_t)J.cap + 1u), "label: the record table");
    /* 0: begin */
    hvq_lb_head_begin(J);
    /* 1: the tiles */
    const uint32_t unstored = 0x7EEEEEEEu;
    for (uint32_t i = 0; i < N; ++i) L[i] = unstored;
    std::vector<uint32_t> P(HVQ_LB_TILE);
    std::vector<uint8_t> stored(N, 0);
    for (uint32_t t = 0; t < J.tx * J.ty; ++t) {
        std::fill(P.begin(), P.end(), 0xEEEEEEEEu);
        EACH_LANE(HVQ_LB_LANES) hvq_lb_tile_load(J, t, lane, P.data());
        EACH_LANE(HVQ_LB_LANES) if (!hvq_lb_tile_merge(J, lane, P.data())) hvq_lb_head_status(J);
        EACH_LANE(HVQ_LB_LANES) {
            uint32_t x, y;
            if (!hvq_lb_tile_store(J, t, lane, P.data())) hvq_lb_head_status(J);
            if (hvq_lb_tile_at(J, t, lane, &x, &y))
                for (uint32_t s = 0; s < 4u; ++s) ++stored[y * J.nx + x + s];
        }
    }
    for (uint32_t i = 0; i < N; ++i)
        if (stored[i] != 1 || L[i] == unstored || L[i] > i + 1u) fake_die("label: job %d: element %u of the map was stored %u times by the tiles and holds %#x", k, i, stored[i], L[i]);
    /* 2: the seams */
    for (uint32_t wg = 0; wg * HVQ_LB_LANES < J.seams; ++wg)
        EACH_LANE(HVQ_LB_LANES) if (!hvq_lb_seam(J, wg * HVQ_LB_LANES + lane)) hvq_lb_head_status(J);
    /* 3: flatten (a plane without seams has neither launch) */
    if (max_seams)
        for (uint32_t c = 0; c < J.chunks; ++c) EACH_LANE(HVQ_LB_LANES) if (!hvq_lb_flatten(J, c, lane)) hvq_lb_head_status(J);
    for (uint32_t i = 0; i < N; ++i)
        if (L[i] > i + 1u) fake_die("label: job %d: element %u of the map holds %#x behind the seams: a parent above its child", k, i, L[i]);
    /* 4: the numbers */
    uint32_t base = 0, F = 0;
    std::vector<uint32_t> mask(HVQ_LB_LANES), fg(HVQ_LB_LANES, 0);
    for (uint32_t r = 0; r < (N + HVQ_LB_SPAN - 1u) / HVQ_LB_SPAN; ++r) {
        EACH_LANE(HVQ_LB_LANES) mask[lane] = hvq_lb_number_count(J, r, lane, &fg[lane]);
        uint32_t before = base;
        EACH_LANE(HVQ_LB_LANES) {                                                  /* the scan: the roots of the lanes before */
            hvq_lb_number_store(J, r, lane, mask[lane], before);
            before += (uint32_t)__builtin_popcount(mask[lane]);
        }
        base = before;
    }
    EACH_LANE(HVQ_LB_LANES) F += fg[lane];
    hvq_lb_head_counts(J, base, F);
    /* 5: resolve, 6: finish */
    const uint32_t stored_rows = C[0] < J.cap ? (uint32_t)C[0] : J.cap;
    for (uint32_t c = 0; c < J.chunks; ++c)
        EACH_LANE(HVQ_LB_LANES) {
            HvqLbRec R;
            if (!hvq_lb_resolve(J, c, lane, stored_rows, &R)) hvq_lb_head_status(J);
            hvq_lb_rec_flush(J, stored_rows, &R);
        }
    for (uint32_t c = 0; c < J.chunks; ++c) EACH_LANE(HVQ_LB_LANES) hvq_lb_finish(J, c, lane);
    for (uint32_t i = 0; i < N; ++i)
        if (L[i] > base) fake_die("label: job %d: element %u of the map holds %#x behind the last launch, K is %u", k, i, L[i], base);
}

extern "C" hipError_t hvq_launch_label(const void *jobs_dev, int npics, uint32_t max_tiles, uint32_t max_seams, uint32_t max_chunks, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles || !max_chunks) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_label: one grid row per picture */
    return fake_enqueue(stream, "label", [=]() {
        const HvqLabelJob *jobs = (const HvqLabelJob *)fake_span(jobs_dev, (size_t)npics * sizeof(HvqLabelJob), "label: the job records");
        for (int k = 0; k < npics; ++k) label_picture(k, jobs[k], max_tiles, max_seams, max_chunks);
    });
}

extern "C" hipError_t hvq_launch_select(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_select: one grid row per picture */
    return fake_enqueue(stream, "select", [=]() {
        const int njobs = 3 * npics;
        const HvqSelectJob *jobs = (const HvqSelectJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqSelectJob), "select: the job records");
        for (int k = 0; k < njobs; ++k) {
            const HvqSelectJob &J = jobs[k];
            const bool select = J.body == HVQ_SL_SELECT;
            if (!J.dwords || J.dwords > (1u << 24) || !J.dst || (J.dst & 3u) || J.body > HVQ_SL_SELECT || (k % 3 == 0) != select)
                fake_die("select: job %d: %u dwords to %#llx, body %u", k, J.dwords, (unsigned long long)J.dst, J.body);
            const uint32_t range[6] = { J.area_min, J.area_max, J.w_min, J.w_max, J.h_min, J.h_max };
            const HvqSelectJob A = hvq_sl_job(J.labels, J.comps, J.dst, J.dwords * 4u, 1u, J.cap, select, range, J.invert);
            if (memcmp(&A, &J, sizeof J)) fake_die("select: job %d: the record is not hvq_sl_job's for %u dwords", k, J.dwords);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("select: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            uint32_t stored_rows = 0;
            if (select) {
                if ((J.labels & 15u) || (J.comps & 15u) || J.invert > 1u) fake_die("select: job %d: the map at %#llx, the records at %#llx, invert %u", k,
                                                                                   (unsigned long long)J.labels, (unsigned long long)J.comps, J.invert);
                fake_span((const void *)(uintptr_t)J.labels, 16u * (size_t)J.dwords, "select: the map");
                const uint64_t *C = (const uint64_t *)fake_span((const void *)(uintptr_t)J.comps, 64u * ((size_t)J.cap + 1u), "select: the record table");
                stored_rows = C[1] < J.cap ? (uint32_t)C[1] : J.cap;
            }
            uint32_t *out = (uint32_t *)fake_span((const void *)(uintptr_t)J.dst, 4u * (size_t)J.dwords, "select: the target plane");
            std::vector<uint8_t> stored(J.dwords, 0);
            for (uint32_t t = 0; t < J.tiles; ++t)
                EACH_LANE(HVQ_MP_LANES)
                    for (uint32_t u = 0; u < HVQ_MP_PER; ++u) {
                        const uint32_t d = hvq_mp_dword(t, lane, u);
                        if (d >= J.dwords) continue;
                        out[d] = select ? hvq_sl_dword(J, stored_rows, d) : 0x80808080u;
                        ++stored[d];
                    }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("select: job %d: target dword %zu was stored %u times", k, i, stored[i]);
        }
    });
}
