/*
 * tests/native/fake_corner.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_corner (hvqm4_amd/csrc/hvq_corner.hip) for the CPU
 * fake device.  Linked into the corner driver only (tests/test_corner_cpu.py); the other drivers link without it, and the runtime's weak
 * reference then makes hvq_corner_pictures refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grids of the four launches the way the
 * kernels do, lane by lane, with the functions of hvq_corner.h (HVQ_CR_PLAIN).  Every job record is checked against hvq_cr_job's
 * arithmetic, and the plane, the mask's planes, the list, the row index and the response map must each lie inside one live allocation
 * (fake_span) before a lane touches them.  A tile runs over an array of the kernel's LDS size on the heap, filled with a pattern before
 * every tile (the sanitised build sees an index outside it); the phases run one behind the other where the kernel has its barriers.
 * Every dword of the mask picture must be stored exactly once: a count per dword is kept over the tiles and the fill tiles.  Launch 2
 * and 4 walk a row in batches of 64 dwords with plain counts: the kernels' ballots and the prefix of the lanes below (corner_ballots)
 * are the kernels' own and run on the GPU only; what is shared with them is hvq_cr_mask_dword, hvq_cr_count_store and hvq_cr_emit.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HVQ_CR_PLAIN 1
#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_corner.h"

#define EACH_LANE(n) for (uint32_t lane = 0; lane < (n); ++lane)

static void corner_picture(int k, const HvqCornerJob &J, uint32_t max_tiles, uint32_t max_rows)
{
    if (!J.nx || !J.ny || (J.nx & 3u) || (uint64_t)J.nx * J.ny > (1u << 26) || (J.src & 3u) || !J.mask || (J.mask & 3u) || !J.points || (J.points & 15u) ||
        !J.rows || (J.rows & 15u) || (J.response & 15u) || !J.fill[0] || !J.fill[1] || ((J.fill[0] | J.fill[1]) & 3u))
        fake_die("corner: job %d: a plane of %u x %u at %#llx, mask %#llx, points %#llx, rows %#llx, response %#llx", k, J.nx, J.ny, (unsigned long long)J.src,
                 (unsigned long long)J.mask, (unsigned long long)J.points, (unsigned long long)J.rows, (unsigned long long)J.response);
    if (J.mode > HVQ_CR_MIN_EIGEN || J.radius < 1u || J.radius > HVQ_CR_MAX_R || J.k > 64u || (J.mode == HVQ_CR_MIN_EIGEN && J.k) || J.nms > HVQ_CR_MAX_NMS ||
        J.margin > 255u || J.threshold < 1 || J.cap > (1u << 20))
        fake_die("corner: job %d: mode %u, radius %u, k %u, nms %u, margin %u, threshold %lld, cap %u", k, J.mode, J.radius, J.k, J.nms, J.margin, (long long)J.threshold, J.cap);
    if (J.tx != (J.nx + HVQ_CR_TX - 1u) / HVQ_CR_TX || J.ty != (J.ny + HVQ_CR_TY - 1u) / HVQ_CR_TY) fake_die("corner: job %d: %u x %u tiles for %u x %u", k, J.tx, J.ty, J.nx, J.ny);
    for (uint32_t f = 0; f < 2u; ++f)
        if (!J.fill_dwords[f] || J.fill_tiles[f] != (J.fill_dwords[f] + HVQ_CR_FILL - 1u) / HVQ_CR_FILL || (J.fill_value[f] != 0u && J.fill_value[f] != 0x80808080u))
            fake_die("corner: job %d: fill %u: %u dwords, %u tiles, value %#x", k, f, J.fill_dwords[f], J.fill_tiles[f], J.fill_value[f]);
    if (hvq_cr_tiles(J) > max_tiles || J.ny > max_rows) fake_die("corner: job %d needs %u tiles and %u rows; the grids have %u, %u", k, hvq_cr_tiles(J), J.ny, max_tiles, max_rows);
    const uint32_t N = J.nx * J.ny, dwords = N >> 2;
    fake_span((const void *)(uintptr_t)J.src, N, "corner: the plane");
    uint32_t *M = (uint32_t *)fake_span((const void *)(uintptr_t)J.mask, N, "corner: the mask's analysed plane");
    uint32_t *F[2];
    for (uint32_t f = 0; f < 2u; ++f) F[f] = (uint32_t *)fake_span((const void *)(uintptr_t)J.fill[f], 4u * (size_t)J.fill_dwords[f], "corner: a filled plane of the mask");
    int64_t *P = (int64_t *)fake_span((const void *)(uintptr_t)J.points, 32u * ((size_t)J.cap + 1u), "corner: the list");
    uint32_t *rows = (uint32_t *)fake_span((const void *)(uintptr_t)J.rows, 4u * ((size_t)J.ny + 1u), "corner: the row index");
    if (J.response) fake_span((const void *)(uintptr_t)J.response, 8u * (size_t)N, "corner: the response map");
    /* 1: the tiles, then the fill tiles */
    const uint32_t unstored = 0x7E7E7E7Eu;
    for (uint32_t i = 0; i < dwords; ++i) M[i] = unstored;
    for (uint32_t f = 0; f < 2u; ++f) for (uint32_t i = 0; i < J.fill_dwords[f]; ++i) F[f][i] = unstored;
    std::vector<uint32_t> L(HVQ_CR_LDS);
    for (uint32_t t = 0; t < J.tx * J.ty; ++t) {
        std::fill(L.begin(), L.end(), 0xEEEEEEEEu);
        EACH_LANE(HVQ_CR_LANES) hvq_cr_stage(J, t, lane, L.data());
        EACH_LANE(HVQ_CR_LANES) hvq_cr_gradients(J, lane, L.data());
        EACH_LANE(HVQ_CR_LANES) hvq_cr_hsums(J, lane, L.data());
        EACH_LANE(HVQ_CR_LANES) hvq_cr_responses(J, t, lane, L.data());
        EACH_LANE(HVQ_CR_LANES) {
            int32_t x0, y0;
            hvq_cr_tile_at(J, t, &x0, &y0);
            const uint32_t x = (uint32_t)x0 + (lane & 15u) * 4u, y = (uint32_t)y0 + (lane >> 4);
            if (x < J.nx && y < J.ny && M[(y * J.nx + x) >> 2] != unstored) fake_die("corner: job %d: dword %u of the mask is stored twice", k, (y * J.nx + x) >> 2);
            hvq_cr_suppress(J, t, lane, L.data());
        }
    }
    for (uint32_t f = 0; f < 2u; ++f)
        for (uint32_t t = 0; t < J.fill_tiles[f]; ++t) EACH_LANE(HVQ_CR_LANES) hvq_cr_fill(J, f, t, lane);
    for (uint32_t i = 0; i < dwords; ++i)
        if ((M[i] & 0x01010101u) * 255u != M[i])                                    /* every byte 0 or 255; the pattern is neither */
            fake_die("corner: job %d: dword %u of the mask holds %#x behind the tiles", k, i, M[i]);
    for (uint32_t f = 0; f < 2u; ++f)
        for (uint32_t i = 0; i < J.fill_dwords[f]; ++i)
            if (F[f][i] != J.fill_value[f]) fake_die("corner: job %d: dword %u of filled plane %u holds %#x", k, i, f, F[f][i]);
    /* 2: a wave a row counts */
    for (uint32_t y = 0; y < J.ny; ++y) {
        uint32_t count = 0;
        for (uint32_t d0 = 0; d0 < (J.nx >> 2); d0 += 64u)
            EACH_LANE(64u) count += (uint32_t)__builtin_popcount(hvq_cr_mask_dword(J, y, d0 + lane) & 0x01010101u);
        hvq_cr_count_store(J, y, count);
    }
    /* 3: the scan */
    std::vector<uint32_t> mine(HVQ_CR_LANES);
    EACH_LANE(HVQ_CR_LANES) mine[lane] = hvq_cr_scan_sum(J, lane);
    uint32_t before = 0;
    EACH_LANE(HVQ_CR_LANES) { hvq_cr_scan_store(J, lane, before); before += mine[lane]; }
    hvq_cr_head(J, before);
    /* 4: a wave a row places its corners */
    for (uint32_t y = 0; y < J.ny; ++y) {
        uint32_t base = rows[y];
        if (rows[y + 1u] < base) fake_die("corner: job %d: the row index descends at row %u", k, y);
        if (rows[y + 1u] == base || base >= J.cap) continue;
        for (uint32_t d0 = 0; d0 < (J.nx >> 2); d0 += 64u)
            EACH_LANE(64u) {
                const uint32_t v = hvq_cr_mask_dword(J, y, d0 + lane);
                for (uint32_t s = 0; s < 4u; ++s)
                    if ((v >> (8u * s)) & 1u) hvq_cr_emit(J, 4u * (d0 + lane) + s, y, ++base);
            }
        if (base != rows[y + 1u]) fake_die("corner: job %d: row %u placed %u corners, the index says %u", k, y, base - rows[y], rows[y + 1u] - rows[y]);
    }
    if (P[0] != (int64_t)before || rows[J.ny] != before) fake_die("corner: job %d: K is %u, the list says %lld, the index %u", k, before, (long long)P[0], rows[J.ny]);
}

extern "C" hipError_t hvq_launch_corner(const void *jobs_dev, int npics, uint32_t max_tiles, uint32_t max_rows, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles || !max_rows) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_corner: one grid row per picture */
    return fake_enqueue(stream, "corner", [=]() {
        const HvqCornerJob *jobs = (const HvqCornerJob *)fake_span(jobs_dev, (size_t)npics * sizeof(HvqCornerJob), "corner: the job records");
        for (int k = 0; k < npics; ++k) corner_picture(k, jobs[k], max_tiles, max_rows);
    });
}
