/*
 * tests/native/fake_filter.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_filter (hvqm4_amd/csrc/hvq_filter.hip) for the CPU
 * fake device.  Linked into the filter driver only (tests/test_filters_cpu.py); the other drivers link without it, and the runtime's
 * weak reference then makes hvq_filter_pictures refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_filter_kernel does --
 * planes x tiles, and within a tile of the filter body its phases lane by lane (the staged rows as aligned dwords, per term the
 * horizontal sums of a wave's rows and the vertical walk under a lane's four target rows, the tile's bytes, a dword a lane) or the four
 * dwords a lane of the copy body, with the kernel's own index arithmetic of hvq_filter.h -- and reaches every byte of the pictures through
 * fake_span at that moment.  The LDS arrays are vectors of the kernel's sizes, every index checked; an entry that was not written in
 * this tile may not be read.  Every target byte must be stored exactly once: a map of the plane counts the stores.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_filter.h"

namespace {

struct Lds {
    std::vector<uint32_t> raw = std::vector<uint32_t>(HVQ_FL_MAX_ROWS * HVQ_FL_ROW_DWORDS);
    std::vector<int32_t> hs[2] = { std::vector<int32_t>(HVQ_FL_MAX_ROWS * 64u), std::vector<int32_t>(HVQ_FL_MAX_ROWS * 64u) };
    std::vector<uint8_t> raw_set = std::vector<uint8_t>(HVQ_FL_MAX_ROWS * HVQ_FL_ROW_DWORDS), hs_set[2] = { std::vector<uint8_t>(HVQ_FL_MAX_ROWS * 64u), std::vector<uint8_t>(HVQ_FL_MAX_ROWS * 64u) };
    uint8_t out[HVQ_FL_TH][HVQ_FL_TW];
    void clear()
    {
        std::fill(raw_set.begin(), raw_set.end(), 0);
        for (auto &v : hs_set) std::fill(v.begin(), v.end(), 0);
        memset(out, 0xEE, sizeof out);
    }
    void raw_put(size_t i, uint32_t v) { if (i >= raw.size()) fake_die("filter: staged dword %zu is outside the LDS array", i); raw[i] = v; raw_set[i] = 1; }
    uint8_t raw_byte(size_t i)
    {
        if (i >= raw.size() * 4u) fake_die("filter: staged byte %zu is outside the LDS array", i);
        if (!raw_set[i >> 2]) fake_die("filter: staged byte %zu is read but was not staged", i);
        return ((const uint8_t *)raw.data())[i];
    }
    void hs_put(int t, size_t i, int32_t v) { if (i >= hs[t].size()) fake_die("filter: horizontal sum %zu is outside the LDS array", i); hs[t][i] = v; hs_set[t][i] = 1; }
    int32_t hs_get(int t, size_t i)
    {
        if (i >= hs[t].size()) fake_die("filter: horizontal sum %zu is outside the LDS array", i);
        if (!hs_set[t][i]) fake_die("filter: horizontal sum %zu of term %d is read but was not made", i, t);
        return hs[t][i];
    }
};

int64_t checked(int64_t v, int k)
{
    if (v < -(int64_t)2147483647 - 1 || v > 2147483647) fake_die("filter: job %d: a sum of %lld leaves 32 bits", k, (long long)v);
    return v;
}

/* one term of the filter body: every lane of the workgroup, phase by phase */
void term_pass(const HvqFilterTermDev &T, int t, int k, uint32_t c0, uint32_t nx, uint32_t rows, uint32_t rmax, Lds &L, int64_t (*cell)[4])
{
    if (T.rx < 0 || T.rx > (int32_t)HVQ_FL_MAX_R || T.ry < 0 || T.ry > (int32_t)rmax) fake_die("filter: job %d: term %d has radii %d, %d (rmax %u)", k, t, T.rx, T.ry, rmax);
    const uint32_t rx = (uint32_t)T.rx, ry = (uint32_t)T.ry;
    const uint32_t U = rows <= 24u ? 6u : 12u;                                       /* the staged rows a wave makes the sums of */
    if (rows > 4u * U) fake_die("filter: job %d: %u staged rows, a wave makes the sums of %u at the most", k, rows, U);
    for (uint32_t lane = 0; lane < HVQ_FL_LANES; ++lane) {                           /* horizontal sums: wave g the staged rows g, g + 4, ... */
        const uint32_t cl = lane & 63u, g = lane >> 6;
        int64_t acc[12] = { 0 };
        for (uint32_t i = 0; i <= 2u * rx; ++i) {
            const int32_t w = T.wx[i];
            if (!w) continue;
            const uint32_t off = hvq_fl_tap_byte(c0, c0 + cl, i, rx, nx);
            if (off >= HVQ_FL_ROW_DWORDS * 4u) fake_die("filter: job %d: tap %u of column %u meets byte %u of a staged row", k, i, c0 + cl, off);
            for (uint32_t u = 0; u < U; ++u)                                         /* a row past the staged ones: the last one, its sum is not stored */
                acc[u] = checked(acc[u] + (int64_t)w * L.raw_byte((size_t)std::min(g + 4u * u, rows - 1u) * HVQ_FL_ROW_DWORDS * 4u + off), k);
        }
        for (uint32_t u = 0; u < U; ++u)
            if (g + 4u * u < rows) L.hs_put(t, (size_t)(g + 4u * u) * 64u + cl, (int32_t)acc[u]);
    }
    for (uint32_t lane = 0; lane < HVQ_FL_LANES; ++lane) {                           /* the vertical walk, four rows a step */
        const uint32_t cl = lane & 63u, g = lane >> 6;
        const size_t base = (size_t)(4u * g + rmax - ry) * 64u + cl;
        const uint32_t last = 3u + 2u * ry;
        for (uint32_t m0 = 0; m0 <= last; m0 += 4u)
            for (uint32_t q = 0; q < 4u; ++q) {
                const int32_t h = L.hs_get(t, base + (size_t)std::min(m0 + q, last) * 64u);
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t kk = m0 + q - j;
                    const int32_t w = kk <= 2u * ry ? T.wy[kk & 31u] : 0;
                    cell[lane][j] = checked(cell[lane][j] + (int64_t)w * h, k);
                }
            }
    }
}

void filter_tile(const HvqFilterJob &J, const HvqFilterPlaneDev &F, int k, uint32_t c0, uint32_t r0, Lds &L)
{
    const uint32_t nx = J.nx, ny = J.ny, rmax = (uint32_t)F.rmax, rows = HVQ_FL_TH + 2u * rmax;
    for (uint32_t lane = 0; lane < HVQ_FL_LANES; ++lane)                             /* (1) stage */
        for (uint32_t u = 0; u < 5u; ++u) {
            const uint32_t idx = lane + HVQ_FL_LANES * u, rr = idx / HVQ_FL_ROW_DWORDS, kd = idx - rr * HVQ_FL_ROW_DWORDS;
            if (rr >= rows) continue;
            const uint32_t y = hvq_fl_stage_row(r0, rr, rmax, ny), d = hvq_fl_stage_dword(c0, kd, nx);
            if (y >= ny || d >= (nx >> 2)) fake_die("filter: job %d: staged dword %u of row %u leaves the %u x %u plane", k, d, y, nx, ny);
            uint32_t v;
            memcpy(&v, fake_span((const void *)(uintptr_t)(J.src + ((uint64_t)y * (nx >> 2) + d) * 4u), 4, "filter: a dword of a staged source row"), 4);
            L.raw_put(idx, v);
        }
    static int64_t t0[HVQ_FL_LANES][4], t1[HVQ_FL_LANES][4];
    memset(t0, 0, sizeof t0);
    memset(t1, 0, sizeof t1);
    term_pass(F.term[0], 0, k, c0, nx, rows, rmax, L, t0);
    if (F.terms == 2) term_pass(F.term[1], 1, k, c0, nx, rows, rmax, L, t1);
    for (uint32_t lane = 0; lane < HVQ_FL_LANES; ++lane)
        for (uint32_t j = 0; j < 4u; ++j) {
            const int64_t a = t0[lane][j], b = t1[lane][j];
            const int64_t s = F.combine == 0 ? a + b : F.combine == 1 ? (a + b < 0 ? -(a + b) : a + b) : (a < 0 ? -a : a) + (b < 0 ? -b : b);
            checked(s + F.half, k);
            L.out[(lane >> 6) * 4u + j][lane & 63u] = (uint8_t)hvq_fl_finish((int32_t)a, (int32_t)b, F.combine, F.half, F.shift, F.bias);
        }
}

void copy_tile(const HvqFilterJob &J, uint32_t c0, uint32_t r0, uint8_t (*out)[HVQ_FL_CTW])
{
    for (uint32_t lane = 0; lane < HVQ_FL_LANES; ++lane) {
        const uint32_t col = c0 + (lane & 63u) * 4u, rb = r0 + (lane >> 6);
        if (col >= J.nx) continue;
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint32_t r = rb + 4u * s;
            if (r >= J.ny) continue;
            memcpy(&out[r - r0][col - c0], fake_span((const void *)(uintptr_t)(J.src + (uint64_t)r * J.nx + col), 4, "filter: a dword of the source row"), 4);
        }
    }
}

}

extern "C" hipError_t hvq_launch_filter(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_filter: one grid row per picture */
    return fake_enqueue(stream, "filter", [=]() {
        const int njobs = 3 * npics;
        const HvqFilterJob *jobs = (const HvqFilterJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqFilterJob), "filter: the job records");
        uint32_t npf = 0;
        for (int k = 0; k < njobs; ++k) npf = std::max(npf, jobs[k].pf + 1u);
        if (npf > 128u) fake_die("filter: a job names plane filter %u", npf - 1u);
        const HvqFilterPlaneDev *tab = (const HvqFilterPlaneDev *)fake_span(jobs + njobs, (size_t)npf * sizeof(HvqFilterPlaneDev), "filter: the filter table behind the jobs");
        Lds L;
        std::vector<uint8_t> ctile((size_t)HVQ_FL_CTH * HVQ_FL_CTW);
        for (int k = 0; k < njobs; ++k) {
            const HvqFilterJob &J = jobs[k];
            if (!J.nx || !J.ny || J.nx > 8192u || J.ny > 8192u || (J.nx & 3u) || (J.dst & 3u) || (J.src & 3u))
                fake_die("filter: job %d: %u x %u from %#llx to %#llx", k, J.nx, J.ny, (unsigned long long)J.src, (unsigned long long)J.dst);
            if (J.body != HVQ_FL_FILTER && J.body != HVQ_FL_COPY) fake_die("filter: job %d: body %u", k, J.body);
            const HvqFilterPlaneDev &F = tab[J.pf];
            const bool copy = J.body == HVQ_FL_COPY;
            if (copy && !hvq_fl_is_identity(&F)) fake_die("filter: job %d: the copy body for a filter that is not the identity", k);
            const HvqFilterJob W = hvq_fl_job(J.src, J.dst, J.nx, J.ny, J.pf, copy);
            if (W.tiles_x != J.tiles_x || W.tiles != J.tiles) fake_die("filter: job %d: the tiles do not describe %u x %u", k, J.nx, J.ny);
            if (F.terms != 1 && F.terms != 2) fake_die("filter: job %d: %d terms", k, F.terms);
            if (F.shift < 0 || F.shift > 22 || F.half != (F.shift ? 1 << (F.shift - 1) : 0) || F.combine < 0 || F.combine > 2 || F.rmax < 0 || F.rmax > (int32_t)HVQ_FL_MAX_R)
                fake_die("filter: job %d: shift %d, half %d, combine %d, rmax %d", k, F.shift, F.half, F.combine, F.rmax);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("filter: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            const uint32_t tw = copy ? HVQ_FL_CTW : HVQ_FL_TW, th = copy ? HVQ_FL_CTH : HVQ_FL_TH;
            std::vector<uint8_t> stored((size_t)J.nx * J.ny, 0);
            for (uint32_t t = 0; t < J.tiles; ++t) {                                 /* workgroups past them leave */
                const uint32_t ty = t / J.tiles_x, c0 = (t - ty * J.tiles_x) * tw, r0 = ty * th;
                L.clear();
                memset(ctile.data(), 0xEE, ctile.size());
                if (copy) copy_tile(J, c0, r0, (uint8_t (*)[HVQ_FL_CTW])ctile.data());
                else filter_tile(J, F, k, c0, r0, L);
                for (uint32_t row = r0; row < std::min(r0 + th, J.ny); ++row)        /* every dword of the tile inside the plane: one store */
                    for (uint32_t col = c0; col < std::min(c0 + tw, J.nx); col += 4u) {
                        uint8_t *d = (uint8_t *)fake_span((const void *)(uintptr_t)(J.dst + (uint64_t)row * J.nx + col), 4, "filter: a dword of the target plane");
                        memcpy(d, copy ? &ctile[(size_t)(row - r0) * HVQ_FL_CTW + (col - c0)] : &L.out[row - r0][col - c0], 4);
                        for (uint32_t i = 0; i < 4u; ++i) ++stored[(size_t)row * J.nx + col + i];
                    }
            }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("filter: job %d: target sample %zu was stored %u times", k, i, stored[i]);
        }
    });
}
