/*
 * tests/native/fake_integral.cpp -- TEST INFRASTRUCTURE: the CPU bodies of hvq_launch_integral, hvq_launch_window and hvq_launch_rects
 * (hvqm4_amd/csrc/hvq_integral.hip) for the CPU fake device.  Linked into the integral driver only (tests/test_integral_cpu.py); the
 * other drivers link without it, and the runtime's weak references then make the three calls refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grids of the launches the way the kernels
 * do, lane by lane, with the functions of hvq_integral.h (HVQ_IG_PLAIN).
 *   integral: every job record is checked against hvq_ig_job, and the plane and the tables must each lie inside one live allocation
 *            (fake_span) before a lane touches them.  The tables are filled with a pattern; then the row groups: a wave is 64 values in
 *            an array, a step of the prefix reads the array of the step before -- what the wave's shuffle gives --, and the carry is lane
 *            63's prefix; every element of a row must be stored exactly once.  Then the column groups, every lane; S(Nx - 1, Ny - 1) must
 *            be the plane's sum modulo 2^32 and Q's its sum of squares.
 *   window:  tiles x lanes; every dword of the picture must be stored exactly once.
 *   rects:   the head and the tables are checked, then a lane a rectangle; every triple must be stored.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HVQ_IG_PLAIN 1
#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_integral.h"

#define EACH_LANE(n) for (uint32_t lane = 0; lane < (n); ++lane)

static void integral_picture(int k, const HvqIntegralJob &J, uint32_t max_rows, uint32_t max_cols)
{
    if (!J.nx || !J.ny || (J.nx & 3u) || J.nx > 8192u || J.ny > 8192u || (J.src & 3u) || !J.sums || (J.sums & 15u) || (J.squares & 15u))
        fake_die("integral: job %d: a plane of %u x %u at %#llx, the tables at %#llx, %#llx", k, J.nx, J.ny, (unsigned long long)J.src, (unsigned long long)J.sums,
                 (unsigned long long)J.squares);
    const HvqIntegralJob A = hvq_ig_job(J.src, J.sums, J.squares, J.nx, J.ny);
    if (memcmp(&A, &J, sizeof J)) fake_die("integral: job %d: the record is not hvq_ig_job's for %u x %u", k, J.nx, J.ny);
    if (J.rowgroups > max_rows || J.colgroups > max_cols) fake_die("integral: job %d needs %u row groups and %u column groups; the grids have %u, %u", k, J.rowgroups, J.colgroups, max_rows, max_cols);
    const size_t N = (size_t)J.nx * J.ny;
    const uint8_t *A8 = (const uint8_t *)fake_span((const void *)(uintptr_t)J.src, N, "integral: the plane");
    uint32_t *S = (uint32_t *)fake_span((const void *)(uintptr_t)J.sums, 4u * N, "integral: the table of sums");
    uint64_t *Q = J.squares ? (uint64_t *)fake_span((const void *)(uintptr_t)J.squares, 8u * N, "integral: the table of squares") : nullptr;
    const uint32_t unstored = 0x7EEEEEEEu;
    for (size_t i = 0; i < N; ++i) { S[i] = unstored; if (Q) Q[i] = ~(uint64_t)unstored; }
    /* 1: the rows */
    for (uint32_t g = 0; g < J.rowgroups; ++g)
        for (uint32_t w = 0; w < HVQ_IG_WAVES; ++w) {
            const uint32_t y = g * HVQ_IG_WAVES + w;
            if (y >= J.ny) continue;
            uint32_t carry = 0;
            uint64_t qcarry = 0;
            for (uint32_t c = 0; c < J.chunks; ++c) {
                uint32_t v[HVQ_IG_WAVE], t[HVQ_IG_WAVE], s[HVQ_IG_WAVE], was[HVQ_IG_WAVE];
                uint64_t tq[HVQ_IG_WAVE], q[HVQ_IG_WAVE], qwas[HVQ_IG_WAVE];
                EACH_LANE(HVQ_IG_WAVE) { v[lane] = hvq_ig_row_load(J, y, c, lane); s[lane] = t[lane] = hvq_ig_sum4(v[lane]); q[lane] = tq[lane] = hvq_ig_sq4(v[lane]); }
                for (uint32_t d = 1u; d < HVQ_IG_WAVE; d <<= 1) {
                    memcpy(was, s, sizeof s); memcpy(qwas, q, sizeof q);
                    EACH_LANE(HVQ_IG_WAVE) {
                        s[lane] = hvq_ig_scan_step(was[lane], was[lane >= d ? lane - d : lane], lane, d);       /* a lane without one below gets its own */
                        q[lane] = hvq_ig_scan_step64(qwas[lane], qwas[lane >= d ? lane - d : lane], lane, d);
                    }
                }
                EACH_LANE(HVQ_IG_WAVE) {
                    const uint32_t x = c * HVQ_IG_CHUNK + lane * 4u;
                    if (x < J.nx)
                        for (uint32_t u = 0; u < 4u; ++u)
                            if (S[(size_t)y * J.nx + x + u] != unstored) fake_die("integral: job %d: element (%u, %u) of the table is stored twice by the row pass", k, x + u, y);
                    hvq_ig_row_store(J, y, c, lane, v[lane], carry + s[lane] - t[lane], qcarry + q[lane] - tq[lane]);
                }
                carry += s[HVQ_IG_WAVE - 1u];
                qcarry += q[HVQ_IG_WAVE - 1u];
            }
        }
    for (size_t i = 0; i < N; ++i)
        if (S[i] == unstored || (Q && Q[i] == ~(uint64_t)unstored)) fake_die("integral: job %d: element %zu of a table was not stored by the row pass", k, i);
    /* 2: the columns */
    for (uint32_t g = 0; g < J.colgroups; ++g) EACH_LANE(HVQ_IG_CLANES) hvq_ig_column(J, g, lane);
    uint64_t sum = 0, sq = 0;
    for (size_t i = 0; i < N; ++i) { sum += A8[i]; sq += (uint64_t)A8[i] * A8[i]; }
    if (S[N - 1] != (uint32_t)sum || (Q && Q[N - 1] != sq)) fake_die("integral: job %d: the last element of a table is not the plane's sum", k);
}

extern "C" hipError_t hvq_launch_integral(const void *jobs_dev, int npics, uint32_t max_rowgroups, uint32_t max_colgroups, hipStream_t stream)
{
    if (npics <= 0 || !max_rowgroups || !max_colgroups) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_integral: one grid row per picture */
    return fake_enqueue(stream, "integral", [=]() {
        const HvqIntegralJob *jobs = (const HvqIntegralJob *)fake_span(jobs_dev, (size_t)npics * sizeof(HvqIntegralJob), "integral: the job records");
        for (int k = 0; k < npics; ++k) integral_picture(k, jobs[k], max_rowgroups, max_colgroups);
    });
}

extern "C" hipError_t hvq_launch_window(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_window: one grid row per picture */
    return fake_enqueue(stream, "window", [=]() {
        const HvqWindowJob *jobs = (const HvqWindowJob *)fake_span(jobs_dev, (size_t)npics * sizeof(HvqWindowJob), "window: the job records");
        for (int k = 0; k < npics; ++k) {
            const HvqWindowJob &J = jobs[k];
            if (!J.nx || !J.ny || (J.nx & 3u) || J.nx > 8192u || J.ny > 8192u || (J.src & 3u) || !J.sums || (J.sums & 15u) || (J.squares & 15u) || !J.dst || (J.dst & 15u) ||
                J.mode > HVQ_WN_THRESHOLD || J.rx > 8191u || J.ry > 8191u || J.invert > 1u || J.k < -1024 || J.k > 1024 || J.c < -255 || J.c > 255)
                fake_die("window: job %d: a plane of %u x %u, mode %u, radii %u, %u, k %d, c %d, invert %u", k, J.nx, J.ny, J.mode, J.rx, J.ry, J.k, J.c, J.invert);
            const HvqWindowJob A = hvq_wn_job(J.src, J.sums, J.squares, J.dst, J.nx, J.ny, J.cdwords, J.mode, J.rx, J.ry, J.k, J.c, J.invert);
            if (memcmp(&A, &J, sizeof J)) fake_die("window: job %d: the record is not hvq_wn_job's for %u x %u", k, J.nx, J.ny);
            if (J.tiles > max_tiles) fake_die("window: job %d needs %u tiles, the grid has %u per picture", k, J.tiles, max_tiles);
            if (hvq_wn_needs_squares(J.mode, J.k) && !J.squares) fake_die("window: job %d: mode %u with k %d and no table of squares", k, J.mode, J.k);
            const uint64_t wx = std::min<uint64_t>(2u * (uint64_t)J.rx + 1u, J.nx), wy = std::min<uint64_t>(2u * (uint64_t)J.ry + 1u, J.ny);
            if (wx * wy > HVQ_WN_MAX_AREA) fake_die("window: job %d: a window of %llu samples", k, (unsigned long long)(wx * wy));
            const size_t N = (size_t)J.nx * J.ny, dwords = N / 4u + J.cdwords;
            fake_span((const void *)(uintptr_t)J.src, N, "window: the plane");
            fake_span((const void *)(uintptr_t)J.sums, 4u * N, "window: the table of sums");
            if (J.squares) fake_span((const void *)(uintptr_t)J.squares, 8u * N, "window: the table of squares");
            uint32_t *out = (uint32_t *)fake_span((const void *)(uintptr_t)J.dst, 4u * dwords, "window: the picture written");
            std::vector<uint8_t> stored(dwords, 0);
            for (uint32_t t = 0; t < J.ytiles; ++t)
                EACH_LANE(HVQ_WN_LANES) {
                    uint32_t x, y;
                    hvq_wn_place(J, t, lane, &x, &y);
                    if (x >= J.nx || y >= J.ny) continue;
                    const size_t d = ((size_t)y * J.nx + x) >> 2;
                    out[d] = hvq_wn_dword(J, x, y);
                    ++stored[d];
                }
            for (uint32_t t = 0; t < J.tiles - J.ytiles; ++t)
                EACH_LANE(HVQ_WN_LANES)
                    for (uint32_t u = 0; u < HVQ_WN_PER; ++u) {
                        const uint32_t d = hvq_wn_chroma(t, lane, u);
                        if (d >= J.cdwords) continue;
                        out[N / 4u + d] = 0x80808080u;
                        ++stored[N / 4u + d];
                    }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("window: job %d: target dword %zu was stored %u times", k, i, stored[i]);
        }
    });
}

extern "C" hipError_t hvq_launch_rects(const void *head_dev, int npics, uint32_t nrects, hipStream_t stream)
{
    if (npics <= 0 || !nrects) return hipSuccess;
    return fake_enqueue(stream, "rects", [=]() {
        const HvqRectHead *H = (const HvqRectHead *)fake_span(head_dev, sizeof(HvqRectHead) + (size_t)npics * sizeof(HvqRectTables), "rects: the head and the tables");
        const HvqRectTables *T = (const HvqRectTables *)(H + 1);
        if (H->nrects != nrects || H->npics != (uint32_t)npics || !H->rects || (H->rects & 3u) || !H->dims || (H->dims & 3u) || !H->out || (H->out & 7u))
            fake_die("rects: the head: %u rectangles of %u pictures, the launch has %u, %d", H->nrects, H->npics, nrects, npics);
        fake_span((const void *)(uintptr_t)H->rects, 20u * (size_t)nrects, "rects: the rectangles");
        const uint32_t *D = (const uint32_t *)fake_span((const void *)(uintptr_t)H->dims, 8u * (size_t)npics, "rects: the sizes");
        uint64_t *O = (uint64_t *)fake_span((const void *)(uintptr_t)H->out, 24u * (size_t)nrects, "rects: the results");
        for (int i = 0; i < npics; ++i) {
            if (!T[i].sums || (T[i].sums & 15u) || (T[i].squares & 15u)) fake_die("rects: picture %d: the tables at %#llx, %#llx", i, (unsigned long long)T[i].sums, (unsigned long long)T[i].squares);
            fake_span((const void *)(uintptr_t)T[i].sums, 4u * (size_t)D[2 * i] * D[2 * i + 1], "rects: a table of sums");
            if (T[i].squares) fake_span((const void *)(uintptr_t)T[i].squares, 8u * (size_t)D[2 * i] * D[2 * i + 1], "rects: a table of squares");
        }
        const uint64_t unstored = 0x7EEEEEEE7EEEEEEEull;
        for (size_t i = 0; i < 3u * (size_t)nrects; ++i) O[i] = unstored;
        const uint32_t groups = (nrects + HVQ_RC_LANES - 1u) / HVQ_RC_LANES;
        for (uint32_t g = 0; g < groups; ++g)
            EACH_LANE(HVQ_RC_LANES)
                if (g * HVQ_RC_LANES + lane < H->nrects) hvq_rc_rect(*H, T, g * HVQ_RC_LANES + lane);
        for (size_t i = 0; i < 3u * (size_t)nrects; ++i)
            if (O[i] == unstored) fake_die("rects: element %zu of the results was not stored", i);
    });
}
