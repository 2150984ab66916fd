/*
 * tests/native/fake_map.cpp -- TEST INFRASTRUCTURE: the CPU bodies of hvq_launch_map and hvq_launch_tables (hvqm4_amd/csrc/hvq_map.hip) for
 * the CPU fake device.  Linked into the map driver only (tests/test_map_cpu.py); the other drivers link without it, and the runtime's weak
 * references then make hvq_map_pictures and hvq_histogram_tables refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way the kernels do and reaches every
 * byte through fake_span at that moment -- the tables too, which an earlier launch on the stream may have written.
 *   map:     planes x tiles; in a tile every lane loads its HVQ_MP_PER dwords (hvq_mp_dword of hvq_map.h), the workgroup stages the
 *            plane's table into an array of the kernel's size on the heap (the sanitised build sees an index outside it), every dword goes
 *            through hvq_mp_lookup4, then every lane stores.  All loads of a tile come before its first store, as in the kernel: with
 *            dst == src a tile reads what it overwrites.  Every target byte must be stored exactly once: a map of the plane counts the
 *            stores.  The job is checked against hvq_mp_job.
 *   tables:  records x planes; the phases of hvq_map.h (hvq_tb_*) for every lane in turn where the kernel has a barrier behind them, over
 *            one HvqTbLds on the heap filled with a pattern before every plane.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_map.h"

#define EACH_LANE(n) for (uint32_t lane = 0; lane < (n); ++lane)

extern "C" hipError_t hvq_launch_map(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_map: one grid row per picture */
    return fake_enqueue(stream, "map", [=]() {
        const int njobs = 3 * npics;
        const HvqMapJob *jobs = (const HvqMapJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqMapJob), "map: the job records");
        std::vector<uint32_t> tile(HVQ_MP_TILE);
        std::vector<HvqMpEntry> T(256);
        for (int k = 0; k < njobs; ++k) {
            const HvqMapJob &J = jobs[k];
            if (!J.dwords || J.dwords > (1u << 24) || (J.dst & 3u) || (J.src & 3u) || J.body > HVQ_MP_LOOKUP)
                fake_die("map: job %d: %u dwords from %#llx to %#llx, body %u", k, J.dwords, (unsigned long long)J.src, (unsigned long long)J.dst, J.body);
            const bool lookup = J.body == HVQ_MP_LOOKUP;
            if (lookup ? !J.table || (J.table & 15u) : J.table != 0u) fake_die("map: job %d: body %u with the table at %#llx", k, J.body, (unsigned long long)J.table);
            const HvqMapJob A = hvq_mp_job(J.src, J.dst, J.table, J.dwords * 4u, 1u, lookup);
            if (A.tiles != J.tiles || J.pad[0] || J.pad[1] || J.pad[2]) fake_die("map: job %d: the record is not hvq_mp_job's for %u dwords", k, J.dwords);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("map: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            std::vector<uint8_t> stored(J.dwords, 0);
            for (uint32_t t = 0; t < J.tiles; ++t) {                                 /* workgroups past them leave */
                std::fill(tile.begin(), tile.end(), 0xEEEEEEEEu);
                std::fill(T.begin(), T.end(), (HvqMpEntry)0xEE);
                EACH_LANE(HVQ_MP_LANES)
                    for (uint32_t u = 0; u < HVQ_MP_PER; ++u) {
                        const uint32_t d = hvq_mp_dword(t, lane, u);
                        if (d < J.dwords) memcpy(&tile[u * HVQ_MP_LANES + lane], fake_span((const void *)(uintptr_t)(J.src + 4u * (uint64_t)d), 4, "map: a dword of the source plane"), 4);
                    }
                if (lookup) {
                    const uint8_t *tab = (const uint8_t *)fake_span((const void *)(uintptr_t)J.table, 256, "map: the plane's table");
                    EACH_LANE(HVQ_MP_LANES) T[lane] = tab[lane];
                    EACH_LANE(HVQ_MP_LANES)
                        for (uint32_t u = 0; u < HVQ_MP_PER; ++u) tile[u * HVQ_MP_LANES + lane] = hvq_mp_lookup4(T.data(), tile[u * HVQ_MP_LANES + lane]);
                }
                EACH_LANE(HVQ_MP_LANES)
                    for (uint32_t u = 0; u < HVQ_MP_PER; ++u) {
                        const uint32_t d = hvq_mp_dword(t, lane, u);
                        if (d >= J.dwords) continue;
                        memcpy((void *)fake_span((const void *)(uintptr_t)(J.dst + 4u * (uint64_t)d), 4, "map: a dword of the target plane"), &tile[u * HVQ_MP_LANES + lane], 4);
                        ++stored[d];
                    }
            }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("map: job %d: target dword %zu was stored %u times", k, i, stored[i]);
        }
    });
}

extern "C" hipError_t hvq_launch_tables(const void *jobs_dev, int nrecords, hipStream_t stream)
{
    if (nrecords <= 0) return hipSuccess;
    if (nrecords > 65535) return hipErrorInvalidValue;                              /* hvq_launch_tables: one grid row per record */
    return fake_enqueue(stream, "tables", [=]() {
        const HvqTableJob *jobs = (const HvqTableJob *)fake_span(jobs_dev, (size_t)nrecords * sizeof(HvqTableJob), "tables: the job records");
        std::unique_ptr<HvqTbLds> L(new HvqTbLds);
        for (int k = 0; k < nrecords; ++k) {
            const HvqTableJob &J = jobs[k];
            if (!J.hist || (J.hist & 15u) || !J.out || (J.out & 15u)) fake_die("tables: job %d: from %#llx to %#llx", k, (unsigned long long)J.hist, (unsigned long long)J.out);
            const uint32_t *hist = (const uint32_t *)fake_span((const void *)(uintptr_t)J.hist, 3u * 256u * 4u, "tables: the histogram record");
            uint8_t *out = (uint8_t *)fake_span((const void *)(uintptr_t)J.out, 768, "tables: the table record");
            for (uint32_t p = 0; p < 3u; ++p) {
                const uint32_t kind = J.rule[p ? 1 : 0].kind, a = J.rule[p ? 1 : 0].a, b = J.rule[p ? 1 : 0].b;
                if (kind > HVQ_TB_OTSU || J.rule[p ? 1 : 0].pad) fake_die("tables: job %d: kind %u", k, kind);
                memset(L.get(), 0xEE, sizeof(HvqTbLds));
                if (kind >= HVQ_TB_EQUALIZE) {
                    EACH_LANE(HVQ_TB_LANES) hvq_tb_load(L.get(), lane, hist[256u * p + lane]);
                    for (uint32_t s = 0; s < 8u; ++s) EACH_LANE(HVQ_TB_LANES) hvq_tb_scan(L.get(), lane, s);
                    EACH_LANE(HVQ_TB_LANES) hvq_tb_select(L.get(), lane, kind, a, b);
                    if (kind == HVQ_TB_OTSU)
                        for (uint32_t s = 128u; s; s >>= 1) EACH_LANE(HVQ_TB_LANES) hvq_tb_reduce(L.get(), lane, s);
                }
                EACH_LANE(HVQ_TB_LANES) out[256u * p + lane] = hvq_tb_value(L.get(), lane, kind, a);
            }
        }
    });
}
