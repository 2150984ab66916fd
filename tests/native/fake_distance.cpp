/*
 * tests/native/fake_distance.cpp -- TEST INFRASTRUCTURE: the CPU bodies of hvq_launch_distance and hvq_launch_distance_mask
 * (hvqm4_amd/csrc/hvq_distance.hip) for the CPU fake device.  Linked into the distance driver only (tests/test_distance_cpu.py); the
 * other drivers link without it, and the runtime's weak references then make hvq_distance_pictures and hvq_distance_mask refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grids of the launches the way the kernels
 * do, lane by lane, with the functions of hvq_distance.h (HVQ_DT_PLAIN).
 *   distance: every job record is checked against hvq_dt_job, and the plane and the map must each lie inside one live allocation
 *            (fake_span) before a lane touches them.  The map is filled with a pattern no pass stores; then the column groups, every lane,
 *            after which no element may hold the pattern and the background is exactly where the map holds 0; then the row groups: the
 *            rounds of staging over an array of the kernel's LDS size on the heap filled with a pattern (the sanitised build sees an index
 *            outside it), and only behind ALL of them -- the kernel's barrier -- the rounds of stores, which must store every element of
 *            the group exactly once.  The rows are overwritten in place: a store that read the map instead of the staged row would read
 *            what an earlier lane left.
 *   mask:    planes x tiles x lanes as in the map launch; every target dword must be stored exactly once.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HVQ_DT_PLAIN 1
#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_map.h"
#include "../../hvqm4_amd/csrc/hvq_distance.h"

#define EACH_LANE(n) for (uint32_t lane = 0; lane < (n); ++lane)

static void distance_picture(int k, const HvqDistanceJob &J, uint32_t max_cols, uint32_t max_rows)
{
    if (!J.nx || !J.ny || (J.nx & 3u) || J.nx > HVQ_DT_SPAN || J.ny > 8192u || (J.src & 3u) || !J.dist || (J.dist & 15u))
        fake_die("distance: job %d: a plane of %u x %u at %#llx, the map at %#llx", k, J.nx, J.ny, (unsigned long long)J.src, (unsigned long long)J.dist);
    if (J.lo > J.hi || J.hi > 255u || J.metric > HVQ_DT_CHESS || J.border > 1u) fake_die("distance: job %d: window %u .. %u, metric %u, border %u", k, J.lo, J.hi, J.metric, J.border);
    const HvqDistanceJob A = hvq_dt_job(J.src, J.dist, J.nx, J.ny, J.lo, J.hi, J.metric, J.border);
    if (memcmp(&A, &J, sizeof J)) fake_die("distance: job %d: the record is not hvq_dt_job's for %u x %u", k, J.nx, J.ny);
    if (J.colgroups > max_cols || J.rowgroups > max_rows || J.rows * J.nx > HVQ_DT_SPAN || !J.rows)
        fake_die("distance: job %d needs %u column groups and %u row groups of %u rows; the grids have %u, %u", k, J.colgroups, J.rowgroups, J.rows, max_cols, max_rows);
    const uint32_t N = J.nx * J.ny;
    const uint8_t *A8 = (const uint8_t *)fake_span((const void *)(uintptr_t)J.src, N, "distance: the plane");
    uint32_t *D = (uint32_t *)fake_span((const void *)(uintptr_t)J.dist, 4u * (size_t)N, "distance: the map");
    /* 1: the columns */
    const uint32_t unstored = 0x7EEEEEEEu;
    for (uint32_t i = 0; i < N; ++i) D[i] = unstored;
    for (uint32_t g = 0; g < J.colgroups; ++g) EACH_LANE(HVQ_DT_CLANES) hvq_dt_column(J, g, lane);
    for (uint32_t i = 0; i < N; ++i) {
        const bool fg = A8[i] >= J.lo && A8[i] <= J.hi;
        if (D[i] == unstored || (D[i] == 0u) == fg || (D[i] != HVQ_DT_NONE && D[i] > J.ny))
            fake_die("distance: job %d: element %u of the map holds %#x behind the column pass (foreground: %d)", k, i, D[i], (int)fg);
    }
    /* 2: the rows */
    std::vector<uint16_t> G(HVQ_DT_SPAN);
    std::vector<uint8_t> stored(N, 0);
    for (uint32_t g = 0; g < J.rowgroups; ++g) {
        std::fill(G.begin(), G.end(), (uint16_t)0xEEEEu);
        const uint32_t n = hvq_dt_row_samples(J, g), rounds = (n + HVQ_DT_LANES * 4u - 1u) / (HVQ_DT_LANES * 4u);
        for (uint32_t r = 0; r < rounds; ++r) EACH_LANE(HVQ_DT_LANES) hvq_dt_row_stage(J, g, r, lane, G.data());
        for (uint32_t r = 0; r < rounds; ++r)
            EACH_LANE(HVQ_DT_LANES) {
                if (J.metric == HVQ_DT_EUCLID2) hvq_dt_row_store<HVQ_DT_EUCLID2>(J, g, r, lane, G.data());
                else if (J.metric == HVQ_DT_CITY) hvq_dt_row_store<HVQ_DT_CITY>(J, g, r, lane, G.data());
                else hvq_dt_row_store<HVQ_DT_CHESS>(J, g, r, lane, G.data());
                for (uint32_t u = 0; u < 4u; ++u) {
                    const uint32_t i = hvq_dt_row_index(r, u, lane);
                    if (i < n) ++stored[g * J.rows * J.nx + i];
                }
            }
    }
    for (uint32_t i = 0; i < N; ++i)
        if (stored[i] != 1) fake_die("distance: job %d: element %u of the map was stored %u times by the row pass", k, i, stored[i]);
}

extern "C" hipError_t hvq_launch_distance(const void *jobs_dev, int npics, uint32_t max_colgroups, uint32_t max_rowgroups, hipStream_t stream)
{
    if (npics <= 0 || !max_colgroups || !max_rowgroups) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_distance: one grid row per picture */
    return fake_enqueue(stream, "distance", [=]() {
        const HvqDistanceJob *jobs = (const HvqDistanceJob *)fake_span(jobs_dev, (size_t)npics * sizeof(HvqDistanceJob), "distance: the job records");
        for (int k = 0; k < npics; ++k) distance_picture(k, jobs[k], max_colgroups, max_rowgroups);
    });
}

extern "C" hipError_t hvq_launch_distance_mask(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_distance_mask: one grid row per picture */
    return fake_enqueue(stream, "distance mask", [=]() {
        const int njobs = 3 * npics;
        const HvqDistMaskJob *jobs = (const HvqDistMaskJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqDistMaskJob), "distance mask: the job records");
        for (int k = 0; k < njobs; ++k) {
            const HvqDistMaskJob &J = jobs[k];
            const bool fill = J.body == HVQ_DM_FILL;
            if (!J.dwords || J.dwords > (1u << 24) || !J.dst || (J.dst & 3u) || J.body > HVQ_DM_FILL || (k % 3 != 0) != fill)
                fake_die("distance mask: job %d: %u dwords to %#llx, body %u", k, J.dwords, (unsigned long long)J.dst, J.body);
            const HvqDistMaskJob A = hvq_dm_job(J.dist, J.dst, J.dwords * 4u, 1u, J.body, J.lo, J.hi, J.invert);
            if (memcmp(&A, &J, sizeof J)) fake_die("distance mask: job %d: the record is not hvq_dm_job's for %u dwords", k, J.dwords);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("distance mask: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            if (!fill) {
                if ((J.dist & 15u) || J.invert > 1u || J.lo > J.hi) fake_die("distance mask: job %d: the map at %#llx, range %u .. %u, invert %u", k, (unsigned long long)J.dist, J.lo, J.hi, J.invert);
                fake_span((const void *)(uintptr_t)J.dist, 16u * (size_t)J.dwords, "distance mask: the map");
            }
            uint32_t *out = (uint32_t *)fake_span((const void *)(uintptr_t)J.dst, 4u * (size_t)J.dwords, "distance mask: the target plane");
            std::vector<uint8_t> stored(J.dwords, 0);
            for (uint32_t t = 0; t < J.tiles; ++t)
                EACH_LANE(HVQ_MP_LANES)
                    for (uint32_t u = 0; u < HVQ_MP_PER; ++u) {
                        const uint32_t d = hvq_mp_dword(t, lane, u);
                        if (d >= J.dwords) continue;
                        out[d] = fill ? 0x80808080u : hvq_dm_dword(J, d);
                        ++stored[d];
                    }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("distance mask: job %d: target dword %zu was stored %u times", k, i, stored[i]);
        }
    });
}
