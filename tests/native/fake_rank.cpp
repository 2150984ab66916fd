/*
 * tests/native/fake_rank.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_rank (hvqm4_amd/csrc/hvq_rank.hip) for the CPU fake
 * device.  Linked into the rank driver only (tests/test_rank_cpu.py); the other drivers link without it, and the runtime's weak
 * reference then makes hvq_rank_pictures refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_rank_kernel does -- planes
 * x tiles, and within a tile the phases of the plane's body, each for every lane in turn where the kernel has a barrier behind it: the
 * staged rows as aligned dwords with the edge sample in the halo, then hvq_rank.h's own phases (the doubling steps of the min/max body
 * between its LDS arrays, the column sorts and selections of the medians) or the four dwords a lane of the copy body -- and reaches every
 * byte of the pictures through fake_span at that moment.  The LDS arrays are a vector of the kernel's size on the heap (the sanitised
 * build sees an index outside it), filled with a pattern before every tile.  Every target byte must be stored exactly once: a map of the
 * plane counts the stores.  The job is checked against hvq_rk_job: the fake walks the body choice of hvq_rank.h.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_rank.h"

namespace {

const uint32_t *span_dword(uint64_t at, const char *what) { return (const uint32_t *)fake_span((const void *)(uintptr_t)at, 4, what); }

void stage(const HvqRankJob &J, int k, uint32_t c0, uint32_t r0, uint32_t r, uint32_t *raw)
{
    const uint32_t rows = HVQ_RK_TH + 2u * r;
    if (rows > HVQ_RK_MAX_ROWS) fake_die("rank: job %d: %u staged rows", k, rows);
    for (uint32_t lane = 0; lane < HVQ_RK_LANES; ++lane)
        for (uint32_t u = 0; u < 5u; ++u) {
            const uint32_t idx = lane + HVQ_RK_LANES * u, rr = idx / HVQ_RK_ROW_DWORDS, kd = idx - rr * HVQ_RK_ROW_DWORDS;
            if (rr >= rows) continue;
            const uint32_t y = hvq_rk_stage_row(r0, rr, r, J.ny), d = hvq_rk_stage_dword(c0, kd, J.nx);
            if (y >= J.ny || d >= (J.nx >> 2)) fake_die("rank: job %d: staged dword %u of row %u leaves the %u x %u plane", k, d, y, J.nx, J.ny);
            uint32_t v;
            memcpy(&v, span_dword(J.src + ((uint64_t)y * (J.nx >> 2) + d) * 4u, "rank: a dword of a staged source row"), 4);
            raw[idx] = hvq_rk_stage_value(v, c0, kd, J.nx);
        }
}

#define EACH_LANE for (uint32_t lane = 0; lane < HVQ_RK_LANES; ++lane)
#define ADVANCE() { smin = dmin; dmin = dmin == P0 ? P1 : P0; smax = dmax; dmax = dmax == Q0 ? Q1 : Q0; }

void minmax_tile(const HvqRankJob &J, int k, uint32_t c0, uint32_t r0, uint32_t *buf, uint32_t *out)
{
    const uint32_t rx = J.rx, ry = J.ry, op = J.op, rows = HVQ_RK_TH + 2u * ry;
    if (op > HVQ_RK_OP_RANGE || rx > HVQ_RK_MAX_R || ry > HVQ_RK_MAX_R) fake_die("rank: job %d: op %u, radii %u, %u in the min/max body", k, op, rx, ry);
    const int do_min = op != HVQ_RK_OP_MAX, do_max = op != HVQ_RK_OP_MIN;
    uint32_t *const P0 = buf + HVQ_RK_BUF, *const P1 = buf + 2u * HVQ_RK_BUF, *const Q0 = buf + 3u * HVQ_RK_BUF, *const Q1 = buf + 4u * HVQ_RK_BUF;
    stage(J, k, c0, r0, ry, buf);
    const uint32_t *smin = buf, *smax = buf;
    uint32_t *dmin = P0, *dmax = Q0;
    uint32_t c;
    const uint32_t wx = 2u * rx + 1u, wy = 2u * ry + 1u;
    HVQ_RK_STEPS(wx, c) {
        EACH_LANE hvq_rk_h_step(lane, rows, c, do_min, do_max, smin, dmin, smax, dmax);
        ADVANCE()
    }
    EACH_LANE hvq_rk_h_last(lane, rows, rx, wx - c, do_min, do_max, smin, dmin, smax, dmax);
    ADVANCE()
    HVQ_RK_STEPS(wy, c) {
        EACH_LANE hvq_rk_v_step(lane, rows, c, do_min, do_max, smin, dmin, smax, dmax);
        ADVANCE()
    }
    EACH_LANE out[lane] = hvq_rk_v_last(lane, wy - c, op, smin, smax);
}

void median_tile(const HvqRankJob &J, int k, uint32_t c0, uint32_t r0, uint32_t *buf, uint32_t *out)
{
    uint32_t *const S = buf + HVQ_RK_BUF;
    if (J.op != HVQ_RK_OP_MEDIAN || J.rx != J.ry || J.rx != (J.body == HVQ_RK_MED3 ? 1u : 2u)) fake_die("rank: job %d: op %u, radii %u, %u in median body %u", k, J.op, J.rx, J.ry, J.body);
    if (J.body == HVQ_RK_MED3) {
        stage(J, k, c0, r0, 1u, buf);
        EACH_LANE hvq_rk_med_sort3(lane, buf, S);
        EACH_LANE out[lane] = hvq_rk_med_select3(lane, S);
    } else {
        stage(J, k, c0, r0, 2u, buf);
        EACH_LANE hvq_rk_med_sort5(lane, buf, S);
        EACH_LANE out[lane] = hvq_rk_med_select5(lane, S);
    }
}

void copy_tile(const HvqRankJob &J, uint32_t c0, uint32_t r0, uint8_t (*out)[HVQ_RK_CTW])
{
    for (uint32_t lane = 0; lane < HVQ_RK_LANES; ++lane) {
        const uint32_t col = c0 + (lane & 63u) * 4u, rb = r0 + (lane >> 6);
        if (col >= J.nx) continue;
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint32_t r = rb + 4u * s;
            if (r >= J.ny) continue;
            memcpy(&out[r - r0][col - c0], span_dword(J.src + (uint64_t)r * J.nx + col, "rank: a dword of the source row"), 4);
        }
    }
}

}

extern "C" hipError_t hvq_launch_rank(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_rank: one grid row per picture */
    return fake_enqueue(stream, "rank", [=]() {
        const int njobs = 3 * npics;
        const HvqRankJob *jobs = (const HvqRankJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqRankJob), "rank: the job records");
        std::vector<uint32_t> lds(5u * HVQ_RK_BUF), tile(HVQ_RK_LANES);
        std::vector<uint8_t> ctile((size_t)HVQ_RK_CTH * HVQ_RK_CTW);
        for (int k = 0; k < njobs; ++k) {
            const HvqRankJob &J = jobs[k];
            if (!J.nx || !J.ny || J.nx > 8192u || J.ny > 8192u || (J.nx & 3u) || (J.dst & 3u) || (J.src & 3u))
                fake_die("rank: job %d: %u x %u from %#llx to %#llx", k, J.nx, J.ny, (unsigned long long)J.src, (unsigned long long)J.dst);
            if (J.body > HVQ_RK_MED5) fake_die("rank: job %d: body %u", k, J.body);
            const bool copy = J.body == HVQ_RK_COPY;
            if (copy && (J.rx || J.ry || J.op == HVQ_RK_OP_RANGE)) fake_die("rank: job %d: the copy body for op %u of radii %u, %u", k, J.op, J.rx, J.ry);
            /* the record is what hvq_rk_job makes of its plane: chosen, or with the copy body switched off */
            const HvqRankJob A = hvq_rk_job(J.src, J.dst, J.nx, J.ny, J.op, J.rx, J.ry, 0), B = hvq_rk_job(J.src, J.dst, J.nx, J.ny, J.op, J.rx, J.ry, 1);
            if (memcmp(&A, &J, sizeof J) && memcmp(&B, &J, sizeof J)) fake_die("rank: job %d: the record is not hvq_rk_job's for %u x %u, op %u, radii %u, %u", k, J.nx, J.ny, J.op, J.rx, J.ry);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("rank: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            const uint32_t tw = copy ? HVQ_RK_CTW : HVQ_RK_TW, th = copy ? HVQ_RK_CTH : HVQ_RK_TH;
            std::vector<uint8_t> stored((size_t)J.nx * J.ny, 0);
            for (uint32_t t = 0; t < J.tiles; ++t) {                                 /* workgroups past them leave */
                const uint32_t ty = t / J.tiles_x, c0 = (t - ty * J.tiles_x) * tw, r0 = ty * th;
                std::fill(lds.begin(), lds.end(), 0xEEEEEEEEu);
                std::fill(tile.begin(), tile.end(), 0xEEEEEEEEu);
                memset(ctile.data(), 0xEE, ctile.size());
                if (copy) copy_tile(J, c0, r0, (uint8_t (*)[HVQ_RK_CTW])ctile.data());
                else if (J.body == HVQ_RK_MINMAX) minmax_tile(J, k, c0, r0, lds.data(), tile.data());
                else median_tile(J, k, c0, r0, lds.data(), tile.data());
                for (uint32_t row = r0; row < std::min(r0 + th, J.ny); ++row)        /* every dword of the tile inside the plane: one store */
                    for (uint32_t col = c0; col < std::min(c0 + tw, J.nx); col += 4u) {
                        uint8_t *d = (uint8_t *)fake_span((const void *)(uintptr_t)(J.dst + (uint64_t)row * J.nx + col), 4, "rank: a dword of the target plane");
                        memcpy(d, copy ? (const void *)&ctile[(size_t)(row - r0) * HVQ_RK_CTW + (col - c0)] : (const void *)&tile[(size_t)(row - r0) * 16u + ((col - c0) >> 2)], 4);
                        for (uint32_t i = 0; i < 4u; ++i) ++stored[(size_t)row * J.nx + col + i];
                    }
            }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("rank: job %d: target sample %zu was stored %u times", k, i, stored[i]);
        }
    });
}
