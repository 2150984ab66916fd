/*
 * tests/native/fake_bilateral.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_bilateral (hvqm4_amd/csrc/hvq_bilateral.hip) for
 * the CPU fake device.  Linked into the bilateral driver only (tests/test_bilateral_cpu.py); the other drivers link without it, and the
 * runtime's weak reference then makes hvq_bilateral_pictures refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_bilateral_kernel does --
 * planes x tiles, and within a tile the staged rows of the source (and of the guide, when the job has one) as aligned dwords with the
 * edge sample in the halo, the plane's range bytes, then hvq_bilateral.h's own walk of a lane over its window for every lane in turn,
 * or the four dwords a lane of the copy body -- and reaches every byte of the pictures and of the parameter sets behind the jobs through
 * fake_span at that moment.  The LDS arrays are vectors of the kernel's sizes on the heap (the sanitised build sees an index outside
 * them), filled with a pattern before every tile.  Every target byte must be stored exactly once: a map of the plane counts the stores.
 * The job is checked against hvq_bl_job: the fake walks the body choice of hvq_bilateral.h.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_bilateral.h"

namespace {

const uint32_t *span_dword(uint64_t at, const char *what) { return (const uint32_t *)fake_span((const void *)(uintptr_t)at, 4, what); }

void stage(const HvqBilateralJob &J, int k, uint64_t plane, uint32_t c0, uint32_t r0, uint32_t *raw)
{
    const uint32_t rows = HVQ_BL_TH + 2u * J.ry;
    for (uint32_t lane = 0; lane < HVQ_BL_LANES; ++lane)
        for (uint32_t u = 0; u < 3u; ++u) {
            const uint32_t idx = lane + HVQ_BL_LANES * u, rr = idx / HVQ_BL_ROW_DWORDS, kd = idx - rr * HVQ_BL_ROW_DWORDS;
            if (rr >= rows) continue;
            const uint32_t y = hvq_bl_stage_row(r0, rr, J.ry, J.ny), d = hvq_bl_stage_dword(c0, kd, J.nx);
            if (y >= J.ny || d >= (J.nx >> 2)) fake_die("bilateral: job %d: staged dword %u of row %u leaves the %u x %u plane", k, d, y, J.nx, J.ny);
            uint32_t v;
            memcpy(&v, span_dword(plane + ((uint64_t)y * (J.nx >> 2) + d) * 4u, "bilateral: a dword of a staged row"), 4);
            raw[idx] = hvq_bl_stage_value(v, c0, kd, J.nx);
        }
}

void copy_tile(const HvqBilateralJob &J, uint32_t c0, uint32_t r0, uint8_t (*out)[HVQ_BL_CTW])
{
    for (uint32_t lane = 0; lane < HVQ_BL_LANES; ++lane) {
        const uint32_t col = c0 + (lane & 63u) * 4u, rb = r0 + (lane >> 6);
        if (col >= J.nx) continue;
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint32_t r = rb + 4u * s;
            if (r >= J.ny) continue;
            memcpy(&out[r - r0][col - c0], span_dword(J.src + (uint64_t)r * J.nx + col, "bilateral: a dword of the source row"), 4);
        }
    }
}

}

extern "C" hipError_t hvq_launch_bilateral(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_bilateral: one grid row per picture */
    return fake_enqueue(stream, "bilateral", [=]() {
        const int njobs = 3 * npics;
        const HvqBilateralJob *jobs = (const HvqBilateralJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqBilateralJob), "bilateral: the job records");
        const uint8_t *sets_dev = (const uint8_t *)jobs_dev + (size_t)njobs * sizeof(HvqBilateralJob);
        std::vector<uint32_t> A(HVQ_BL_BUF), G(HVQ_BL_BUF), range(64), tile(HVQ_BL_LANES);
        std::vector<uint8_t> ctile((size_t)HVQ_BL_CTH * HVQ_BL_CTW);
        for (int k = 0; k < njobs; ++k) {
            const HvqBilateralJob &J = jobs[k];
            if (!J.nx || !J.ny || J.nx > 8192u || J.ny > 8192u || (J.nx & 3u) || (J.dst & 3u) || (J.src & 3u) || (J.guide & 3u))
                fake_die("bilateral: job %d: %u x %u from %#llx to %#llx, guide %#llx", k, J.nx, J.ny, (unsigned long long)J.src, (unsigned long long)J.dst, (unsigned long long)J.guide);
            if (J.body > HVQ_BL_GENERAL || J.rx > HVQ_BL_MAX_R || J.ry > HVQ_BL_MAX_R || J.ps >= 2u * HVQ_BL_MAX_SETS) fake_die("bilateral: job %d: body %u, radii %u, %u, set %u", k, J.body, J.rx, J.ry, J.ps);
            const bool copy = J.body == HVQ_BL_COPY;
            /* the record is what hvq_bl_job makes of its plane: chosen, or with the copy body switched off */
            const HvqBilateralJob X = hvq_bl_job(J.src, J.dst, J.guide, J.nx, J.ny, J.ps, J.rx, J.ry, 0), Y = hvq_bl_job(J.src, J.dst, J.guide, J.nx, J.ny, J.ps, J.rx, J.ry, 1);
            if (memcmp(&X, &J, sizeof J) && memcmp(&Y, &J, sizeof J)) fake_die("bilateral: job %d: the record is not hvq_bl_job's for %u x %u, radii %u, %u", k, J.nx, J.ny, J.rx, J.ry);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("bilateral: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            /* the plane's set behind the jobs: its radii are the job's */
            const uint8_t *set = (const uint8_t *)fake_span(sets_dev + (size_t)J.ps * HVQ_BL_PLANE_BYTES, HVQ_BL_PLANE_BYTES, "bilateral: a plane's parameter set");
            int32_t radii[2];
            memcpy(radii, set, sizeof radii);
            if ((uint32_t)radii[0] != J.rx || (uint32_t)radii[1] != J.ry) fake_die("bilateral: job %d: radii %u, %u, its set has %d, %d", k, J.rx, J.ry, radii[0], radii[1]);
            const uint32_t tw = copy ? HVQ_BL_CTW : HVQ_BL_TW, th = copy ? HVQ_BL_CTH : HVQ_BL_TH;
            std::vector<uint8_t> stored((size_t)J.nx * J.ny, 0);
            for (uint32_t t = 0; t < J.tiles; ++t) {                                 /* workgroups past them leave */
                const uint32_t ty = t / J.tiles_x, c0 = (t - ty * J.tiles_x) * tw, r0 = ty * th;
                std::fill(A.begin(), A.end(), 0xEEEEEEEEu);
                std::fill(G.begin(), G.end(), 0xEEEEEEEEu);
                std::fill(tile.begin(), tile.end(), 0xEEEEEEEEu);
                memset(ctile.data(), 0xEE, ctile.size());
                if (copy) copy_tile(J, c0, r0, (uint8_t (*)[HVQ_BL_CTW])ctile.data());
                else {
                    stage(J, k, J.src, c0, r0, A.data());
                    if (J.guide) stage(J, k, J.guide, c0, r0, G.data());
                    memcpy(range.data(), set + HVQ_BL_RANGE_AT, 256);
                    for (uint32_t lane = 0; lane < HVQ_BL_LANES; ++lane)
                        tile[lane] = hvq_bl_lane(lane, J.rx, J.ry, J.guide != 0, set + HVQ_BL_SPATIAL_AT, A.data(), J.guide ? G.data() : A.data(), (const uint8_t *)range.data());
                }
                for (uint32_t row = r0; row < std::min(r0 + th, J.ny); ++row)        /* every dword of the tile inside the plane: one store */
                    for (uint32_t col = c0; col < std::min(c0 + tw, J.nx); col += 4u) {
                        uint8_t *d = (uint8_t *)fake_span((const void *)(uintptr_t)(J.dst + (uint64_t)row * J.nx + col), 4, "bilateral: a dword of the target plane");
                        memcpy(d, copy ? (const void *)&ctile[(size_t)(row - r0) * HVQ_BL_CTW + (col - c0)] : (const void *)&tile[(size_t)(row - r0) * 16u + ((col - c0) >> 2)], 4);
                        for (uint32_t i = 0; i < 4u; ++i) ++stored[(size_t)row * J.nx + col + i];
                    }
            }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("bilateral: job %d: target sample %zu was stored %u times", k, i, stored[i]);
        }
    });
}
