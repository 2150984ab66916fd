/*
 * tests/native/fake_warp.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_warp (hvqm4_amd/csrc/hvq_warp.hip) for the CPU fake
 * device.  Linked into the warp driver only (tests/test_warp_cpu.py); the other drivers link without it, and the runtime's weak
 * reference then makes hvq_warp_pictures refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_warp_kernel does --
 * planes x tiles, and within a tile its phases lane by lane (in the tiled body the staged box as aligned dwords, then for every lane its
 * four targets: the coordinates as the tile's 64-bit origin plus a 32-bit delta, the clamped taps, the border rule, the finish; the
 * tile's bytes, a dword a lane) with the kernel's own arithmetic of hvq_warp.h -- and reaches every byte of the pictures through
 * fake_span at that moment.  Every staged read must lie inside the source plane, every LDS index inside the staged box and the array;
 * an entry that was not staged in this tile may not be read; a delta must fit 32 bits.  Every target byte must be stored exactly once: a
 * map of the plane counts the stores.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_warp.h"

namespace {

struct Lds {
    std::vector<uint32_t> raw = std::vector<uint32_t>(HVQ_WP_LDS_DWORDS);
    std::vector<uint8_t> raw_set = std::vector<uint8_t>(HVQ_WP_LDS_DWORDS);
    uint8_t out[HVQ_WP_TH][HVQ_WP_TW];
    void clear() { std::fill(raw_set.begin(), raw_set.end(), 0); memset(out, 0xEE, sizeof out); }
    void raw_put(size_t i, uint32_t v) { if (i >= raw.size()) fake_die("warp: staged dword %zu is outside the LDS array", i); raw[i] = v; raw_set[i] = 1; }
    uint8_t raw_byte(size_t i)
    {
        if (i >= raw.size() * 4u) fake_die("warp: staged byte %zu is outside the LDS array", i);
        if (!raw_set[i >> 2]) fake_die("warp: staged byte %zu is read but was not staged", i);
        return ((const uint8_t *)raw.data())[i];
    }
};

int32_t delta32(int64_t v, int k)
{
    if (v < -(int64_t)2147483647 - 1 || v > 2147483647) fake_die("warp: job %d: a delta of %lld leaves 32 bits", k, (long long)v);
    return (int32_t)v;
}

void tile(const HvqWarpJob &J, int k, uint32_t c0, uint32_t r0, Lds &L)
{
    const bool tiled = J.body == HVQ_WP_TILED;
    const uint32_t nx = J.nx, ny = J.ny, pitch = J.pitch;
    HvqWarpBox B = { 0, 0, 0, 0 };
    if (tiled) {                                                                     /* stage the box */
        B = hvq_wp_box(&J, c0, r0);
        if (B.x0 < 0 || B.x1 < B.x0 || B.x1 >= (int32_t)nx || B.y0 < 0 || B.y1 < B.y0 || B.y1 >= (int32_t)ny)
            fake_die("warp: job %d: the box %d .. %d x %d .. %d leaves the %u x %u plane", k, B.x0, B.x1, B.y0, B.y1, nx, ny);
        const uint32_t bw = (uint32_t)(B.x1 >> 2) - (uint32_t)(B.x0 >> 2) + 1u, bh = (uint32_t)(B.y1 - B.y0) + 1u;
        if (bw > pitch || bh > J.rows) fake_die("warp: job %d: a box of %u dwords x %u rows, the job says %u x %u at the most", k, bw, bh, pitch, J.rows);
        const uint32_t total = bh * pitch;
        for (uint32_t base = 0; base < total; base += 4u * HVQ_WP_LANES)
            for (uint32_t lane = 0; lane < HVQ_WP_LANES; ++lane)
                for (uint32_t u = 0; u < 4u; ++u) {
                    const uint32_t idx = base + lane + HVQ_WP_LANES * u, rr = hvq_wp_stage_row(idx, J.pitch_mul), kd = idx - rr * pitch;
                    if (idx >= total) continue;
                    if (rr != idx / pitch) fake_die("warp: job %d: staged dword %u: row %u by the multiplier, %u by division", k, idx, rr, idx / pitch);
                    if (kd >= bw) continue;
                    const uint32_t y = (uint32_t)B.y0 + rr, d = (uint32_t)(B.x0 >> 2) + kd;
                    if (y >= ny || d >= (nx >> 2)) fake_die("warp: job %d: staged dword %u of row %u leaves the %u x %u plane", k, d, y, nx, ny);
                    uint32_t v;
                    memcpy(&v, fake_span((const void *)(uintptr_t)(J.src + ((uint64_t)y * (nx >> 2) + d) * 4u), 4, "warp: a dword of the staged box"), 4);
                    L.raw_put(idx, v);
                }
    }
    const int64_t ou = J.cu + (int64_t)J.au * c0 + (int64_t)J.bu * r0, ov = J.cv + (int64_t)J.av * c0 + (int64_t)J.bv * r0;
    for (uint32_t lane = 0; lane < HVQ_WP_LANES; ++lane) {
        const uint32_t cl = lane & 63u, g = lane >> 6;
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t row = 4u * g + j;
            const int32_t du = delta32((int64_t)J.au * cl + (int64_t)J.bu * row, k), dv = delta32((int64_t)J.av * cl + (int64_t)J.bv * row, k);
            delta32((int64_t)J.au * cl + (int64_t)J.bu * (row + 1u), k);             /* the kernel steps once more behind its last row */
            delta32((int64_t)J.av * cl + (int64_t)J.bv * (row + 1u), k);
            const int32_t u8 = hvq_wp_u8(ou + du, J.su, nx), v8 = hvq_wp_u8(ov + dv, J.sv, ny);
            const int32_t ix = u8 >> 8, iy = v8 >> 8;
            const uint32_t fx = (uint32_t)u8 & 255u, fy = (uint32_t)v8 & 255u;
            const int32_t x0 = hvq_wp_clamp(ix, nx), x1 = hvq_wp_clamp(ix + 1, nx), y0 = hvq_wp_clamp(iy, ny), y1 = hvq_wp_clamp(iy + 1, ny);
            uint32_t t[2][2];
            for (int jj = 0; jj < 2; ++jj)
                for (int ii = 0; ii < 2; ++ii) {
                    const int32_t x = ii ? x1 : x0, y = jj ? y1 : y0;
                    if (tiled) {
                        if (x < B.x0 || x > B.x1 || y < B.y0 || y > B.y1) fake_die("warp: job %d: tap (%d, %d) lies outside the staged box %d .. %d x %d .. %d", k, x, y, B.x0, B.x1, B.y0, B.y1);
                        t[jj][ii] = L.raw_byte(hvq_wp_lds_byte(&B, pitch, x, y));
                    } else {
                        t[jj][ii] = *(const uint8_t *)fake_span((const void *)(uintptr_t)(J.src + (uint64_t)(uint32_t)y * nx + (uint32_t)x), 1, "warp: a tap of the direct body");
                    }
                    if (J.border && (x != ix + ii || y != iy + jj)) t[jj][ii] = J.fill;
                }
            L.out[row][cl] = (uint8_t)hvq_wp_finish(fx, fy, t[0][0], t[0][1], t[1][0], t[1][1]);
        }
    }
}

}

extern "C" hipError_t hvq_launch_warp(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_warp: one grid row per picture */
    return fake_enqueue(stream, "warp", [=]() {
        const int njobs = 3 * npics;
        const HvqWarpJob *jobs = (const HvqWarpJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqWarpJob), "warp: the job records");
        Lds L;
        for (int k = 0; k < njobs; ++k) {
            const HvqWarpJob &J = jobs[k];
            if (!J.nx || !J.ny || J.nx > 8192u || J.ny > 8192u || (J.nx & 3u) || !J.mx || !J.my || J.mx > 8192u || J.my > 8192u || (J.mx & 3u) || (J.dst & 3u) || (J.src & 3u))
                fake_die("warp: job %d: %u x %u from %#llx to %u x %u at %#llx", k, J.nx, J.ny, (unsigned long long)J.src, J.mx, J.my, (unsigned long long)J.dst);
            if (J.body != HVQ_WP_DIRECT && J.body != HVQ_WP_TILED) fake_die("warp: job %d: body %u", k, J.body);
            if ((J.su != 9u && J.su != 10u) || (J.sv != 9u && J.sv != 10u) || J.border > 1u || J.fill > 255u) fake_die("warp: job %d: shifts %u, %u, border %u, fill %u", k, J.su, J.sv, J.border, J.fill);
            for (int32_t a : { J.au, J.bu, J.av, J.bv })
                if (a > 4 * HVQ_WP_MAX_M || a < -4 * HVQ_WP_MAX_M) fake_die("warp: job %d: a step of %d", k, a);
            HvqWarpJob W = J;
            hvq_wp_choose(&W, J.body == HVQ_WP_TILED ? 2 : 1);
            if (W.body != J.body || W.pitch != J.pitch || W.rows != J.rows || W.pitch_mul != J.pitch_mul || !(J.pitch & 1u))
                fake_die("warp: job %d: body %u, pitch %u, rows %u do not describe the map", k, J.body, J.pitch, J.rows);
            if (J.tiles_x != (J.mx + HVQ_WP_TW - 1u) / HVQ_WP_TW || J.tiles != J.tiles_x * ((J.my + HVQ_WP_TH - 1u) / HVQ_WP_TH)) fake_die("warp: job %d: the tiles do not describe %u x %u", k, J.mx, J.my);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("warp: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            std::vector<uint8_t> stored((size_t)J.mx * J.my, 0);
            for (uint32_t t = 0; t < J.tiles; ++t) {                                 /* workgroups past them leave */
                const uint32_t ty = t / J.tiles_x, c0 = (t - ty * J.tiles_x) * HVQ_WP_TW, r0 = ty * HVQ_WP_TH;
                L.clear();
                tile(J, k, c0, r0, L);
                for (uint32_t row = r0; row < std::min(r0 + HVQ_WP_TH, J.my); ++row)  /* every dword of the tile inside the plane: one store */
                    for (uint32_t col = c0; col < std::min(c0 + HVQ_WP_TW, J.mx); col += 4u) {
                        uint8_t *d = (uint8_t *)fake_span((const void *)(uintptr_t)(J.dst + (uint64_t)row * J.mx + col), 4, "warp: a dword of the target plane");
                        memcpy(d, &L.out[row - r0][col - c0], 4);
                        for (uint32_t i = 0; i < 4u; ++i) ++stored[(size_t)row * J.mx + col + i];
                    }
            }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("warp: job %d: target sample %zu was stored %u times", k, i, stored[i]);
        }
    });
}
