/*
 * tests/native/fake_scale.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_scale (hvqm4_amd/csrc/hvq_scale.hip) for the CPU fake
 * device.  Linked into the scale driver only (tests/test_scale_cpu.py); the other drivers link without it, and the runtime's weak
 * reference then makes hvq_scale_pictures refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_scale_kernel does -- planes
 * x tiles, and within a tile the phases of the tiled body (the chunk's rows staged as aligned dwords, the horizontal sums, the vertical
 * pass into the cells of a lane's four rows) or the four samples a lane of the direct body, with the kernel's own index arithmetic -- and
 * reaches every byte of the pictures through fake_span at that moment (the grid row of a picture walks the tiles of its planes Y, U, V).  The two LDS arrays are vectors of the kernel's sizes, every index
 * checked.  Every target byte must be written exactly once: a map of the plane counts the stores.
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_scale.h"

namespace {

struct Lds {
    std::vector<uint32_t> raw = std::vector<uint32_t>(HVQ_SC_RAW_DWORDS), hs = std::vector<uint32_t>(HVQ_SC_MAX_CHUNK * 64u);
    uint8_t out[HVQ_SC_TH][HVQ_SC_TW];
    uint32_t &raw_at(size_t i) { if (i >= raw.size()) fake_die("scale: staged dword %zu is outside the LDS array", i); return raw[i]; }
    uint8_t raw_byte(size_t i) { if (i >= raw.size() * 4u) fake_die("scale: staged byte %zu is outside the LDS array", i); return ((const uint8_t *)raw.data())[i]; }
    uint32_t &hs_at(size_t i) { if (i >= hs.size()) fake_die("scale: horizontal sum %zu is outside the LDS array", i); return hs[i]; }
};

uint32_t tap(uint32_t at, uint32_t m, uint32_t lo, uint32_t hi) { return std::min(at + m, hi) - std::max(at, lo); }

/* the tiled body of one tile: every lane of the workgroup, phase by phase */
void tiled_tile(const HvqScaleJob &J, int k, uint32_t c0, uint32_t r0, bool wide, Lds &L)
{
    const uint32_t nx = J.nx, ny = J.ny, mx = J.mx, my = J.my, rd = J.row_dwords, chunk = J.chunk;
    const uint32_t qx = J.mul_x, sx = J.shift_x, qy = J.mul_y, sy = J.shift_y;
    const uint32_t c_end = std::min(c0 + HVQ_SC_TW, mx), r_end = std::min(r0 + HVQ_SC_TH, my);
    const uint32_t X0 = hvq_sc_first(nx, mx, c0, qx, sx), X1 = hvq_sc_end(nx, mx, c_end - 1u, qx, sx);
    const uint32_t Y0 = hvq_sc_first(ny, my, r0, qy, sy), Y1 = hvq_sc_end(ny, my, r_end - 1u, qy, sy);
    if (X0 != nx * c0 / mx || X1 != (nx * c_end + mx - 1u) / mx || Y0 != ny * r0 / my || Y1 != (ny * r_end + my - 1u) / my)
        fake_die("scale: job %d: the multipliers do not divide by %u and %u", k, mx, my);
    if (X1 > nx || Y1 > ny || X0 >= X1 || Y0 >= Y1) fake_die("scale: job %d: a tile's sources [%u, %u) x [%u, %u) leave the plane", k, X0, X1, Y0, Y1);
    const uint64_t row0 = J.src + X0;
    const uint32_t mis = (uint32_t)row0 & 3u;
    const uint32_t ndw = (mis + (X1 - X0) + 3u) >> 2;
    if (ndw > rd) fake_die("scale: job %d: a tile's row takes %u dwords, the job says %u at the most", k, ndw, rd);
    uint64_t cell[HVQ_SC_LANES][4];
    memset(cell, 0, sizeof cell);
    for (uint32_t cy = Y0; cy < Y1; cy += chunk) {
        const uint32_t rows = std::min(chunk, Y1 - cy);
        for (uint32_t rr = 0; rr < rows; ++rr) {                                     /* (1) the rows' dwords: wave rr & 3, lanes side by side */
            const void *p = fake_span((const void *)(uintptr_t)(row0 - mis + (uint64_t)(cy + rr) * J.pitch), 4u * ndw, "scale: the dwords of a staged source row");
            (void)L.raw_at((size_t)rr * rd + ndw - 1u);
            memcpy(&L.raw_at((size_t)rr * rd), p, 4u * ndw);
        }
        for (uint32_t lane = 0; lane < HVQ_SC_LANES; ++lane) {                       /* (2) horizontal sums */
            const uint32_t cl = lane & 63u, g = lane >> 6, c = c0 + cl;
            const uint32_t xs = c < mx ? hvq_sc_first(nx, mx, c, qx, sx) : 0u, xe = c < mx ? hvq_sc_end(nx, mx, c, qx, sx) : 0u;
            for (uint32_t rr = g; rr < rows; rr += 4u) {
                uint64_t s = 0;
                uint32_t at = mx * xs;
                for (uint32_t x = xs; x < xe; ++x, at += mx) s += (uint64_t)tap(at, mx, nx * c, nx * (c + 1u)) * L.raw_byte((size_t)rr * rd * 4u + mis + (x - X0));
                if (s >> 21) fake_die("scale: job %d: a horizontal sum of %llu does not fit 21 bits", k, (unsigned long long)s);
                L.hs_at((size_t)rr * 64u + cl) = (uint32_t)s;
            }
        }
        for (uint32_t lane = 0; lane < HVQ_SC_LANES; ++lane) {                       /* (3) the vertical pass */
            const uint32_t cl = lane & 63u, g = lane >> 6;
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t r = r0 + g * 4u + j;
                if (r >= my) continue;
                const uint32_t ys = std::max(hvq_sc_first(ny, my, r, qy, sy), cy), ye = std::min(hvq_sc_end(ny, my, r, qy, sy), cy + rows);
                uint32_t at = my * ys;
                for (uint32_t y = ys; y < ye; ++y, at += my) {
                    cell[lane][j] += (uint64_t)tap(at, my, ny * r, ny * (r + 1u)) * L.hs_at((size_t)(y - cy) * 64u + cl);
                    if (!wide && cell[lane][j] >> 32) fake_die("scale: job %d: a cell of 32 bits wraps (255 nx ny = %llu)", k, 255ull * nx * ny);
                }
            }
        }
    }
    const uint64_t half = ((uint64_t)nx * ny) >> 1;
    for (uint32_t lane = 0; lane < HVQ_SC_LANES; ++lane)
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t q = hvq_sc_div(cell[lane][j] + half, J.magic);
            if (q > 255u) fake_die("scale: job %d: a quotient of %u", k, q);
            L.out[(lane >> 6) * 4u + j][lane & 63u] = (uint8_t)q;
        }
}

void direct_tile(const HvqScaleJob &J, int k, uint32_t c0, uint32_t r0, bool wide, uint8_t (*out)[HVQ_SC_DTW])
{
    const uint32_t nx = J.nx, ny = J.ny, mx = J.mx, my = J.my;
    const uint32_t qx = J.mul_x, sx = J.shift_x, qy = J.mul_y, sy = J.shift_y;
    const uint64_t half = ((uint64_t)nx * ny) >> 1;
    for (uint32_t lane = 0; lane < HVQ_SC_LANES; ++lane) {
        const uint32_t col = c0 + (lane & 63u) * 4u, rb = r0 + (lane >> 6);
        if (col >= mx) continue;
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint32_t r = rb + 4u * s;
            if (r >= my) break;
            uint8_t *o = &out[r - r0][col - c0];
            if (nx == mx && ny == my && !(J.src & 3u)) {                             /* identity from an aligned source: the dword as it stands */
                memcpy(o, fake_span((const void *)(uintptr_t)(J.src + (uint64_t)r * J.pitch + col), 4, "scale: a dword of the source row"), 4);
                continue;
            }
            const uint32_t ys = hvq_sc_first(ny, my, r, qy, sy), ye = hvq_sc_end(ny, my, r, qy, sy);
            if (ys != ny * r / my || ye != (ny * (r + 1u) + my - 1u) / my) fake_die("scale: job %d: the multiplier does not divide by %u", k, my);
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t c = col + i;
                const uint32_t xs = hvq_sc_first(nx, mx, c, qx, sx), xe = hvq_sc_end(nx, mx, c, qx, sx);
                if (xs != nx * c / mx || xe != (nx * (c + 1u) + mx - 1u) / mx) fake_die("scale: job %d: the multiplier does not divide by %u", k, mx);
                uint64_t cell = 0;
                uint32_t aty = my * ys;
                for (uint32_t y = ys; y < ye; ++y, aty += my) {
                    const uint8_t *p = (const uint8_t *)fake_span((const void *)(uintptr_t)(J.src + (uint64_t)y * J.pitch + xs), xe - xs, "scale: the taps of a sample in a source row");
                    uint32_t t = 0, at = mx * xs;
                    for (uint32_t x = xs; x < xe; ++x, at += mx) t += tap(at, mx, nx * c, nx * (c + 1u)) * p[x - xs];
                    cell += (uint64_t)tap(aty, my, ny * r, ny * (r + 1u)) * t;
                    if (!wide && cell >> 32) fake_die("scale: job %d: a cell of 32 bits wraps", k);
                }
                const uint32_t q = hvq_sc_div(cell + half, J.magic);
                if (q > 255u) fake_die("scale: job %d: a quotient of %u", k, q);
                o[i] = (uint8_t)q;
            }
        }
    }
}

}

extern "C" hipError_t hvq_launch_scale(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream)
{
    if (npics <= 0 || !max_tiles) return hipSuccess;
    if (npics > 65535) return hipErrorInvalidValue;                                 /* hvq_launch_scale: one grid row per picture */
    return fake_enqueue(stream, "scale", [=]() {
        const int njobs = 3 * npics;
        const HvqScaleJob *jobs = (const HvqScaleJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqScaleJob), "scale: the job records");
        Lds L;
        std::vector<uint8_t> dtile((size_t)HVQ_SC_DTH * HVQ_SC_DTW);
        for (int k = 0; k < njobs; ++k) {
            const HvqScaleJob &J = jobs[k];
            if (!J.nx || !J.ny || !J.mx || !J.my || J.nx > 8192u || J.ny > 8192u || J.mx > 8192u || J.my > 8192u || (J.mx & 3u) || (J.dst & 3u) || (J.pitch & 3u) || J.pitch < J.nx)
                fake_die("scale: job %d: %u x %u (pitch %u) -> %u x %u at %#llx", k, J.nx, J.ny, J.pitch, J.mx, J.my, (unsigned long long)J.dst);
            if (J.nx > HVQ_SC_MAX_RATIO * J.mx || J.ny > HVQ_SC_MAX_RATIO * J.my) fake_die("scale: job %d: a reduction beyond %u", k, HVQ_SC_MAX_RATIO);
            const HvqScaleJob W = hvq_sc_job(J.src, J.pitch, J.nx, J.ny, J.dst, J.mx, J.my, !(J.body & HVQ_SC_TILED));
            if (W.magic != J.magic || W.tiles_x != J.tiles_x || W.tiles != J.tiles || W.chunk != J.chunk || W.row_dwords != J.row_dwords || W.mul_x != J.mul_x || W.shift_x != J.shift_x ||
                W.mul_y != J.mul_y || W.shift_y != J.shift_y || (W.body & HVQ_SC_WIDE) != (J.body & HVQ_SC_WIDE) ||
                (J.body & ~(HVQ_SC_TILED | HVQ_SC_WIDE)) || !J.chunk || J.chunk > HVQ_SC_MAX_CHUNK || (uint64_t)J.chunk * J.row_dwords > HVQ_SC_RAW_DWORDS)
                fake_die("scale: job %d: magic, tiles, chunk, row_dwords or the multipliers do not describe %u x %u -> %u x %u", k, J.nx, J.ny, J.mx, J.my);
            if (k % 3 == 2 && jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles > max_tiles)
                fake_die("scale: picture %d needs %u tiles, the grid has %u per picture", k / 3, jobs[k - 2].tiles + jobs[k - 1].tiles + J.tiles, max_tiles);
            const bool wide = (J.body & HVQ_SC_WIDE) != 0, tiled = (J.body & HVQ_SC_TILED) != 0;
            if (!wide && 255ull * J.nx * J.ny >= (1ull << 32)) fake_die("scale: job %d: cells of 32 bits for 255 nx ny = %llu", k, 255ull * J.nx * J.ny);
            const uint32_t tw = tiled ? HVQ_SC_TW : HVQ_SC_DTW, th = tiled ? HVQ_SC_TH : HVQ_SC_DTH;
            std::vector<uint8_t> stored((size_t)J.mx * J.my, 0);
            for (uint32_t t = 0; t < J.tiles; ++t) {                                 /* workgroups past them leave */
                const uint32_t ty = t / J.tiles_x, c0 = (t - ty * J.tiles_x) * tw, r0 = ty * th;
                memset(L.out, 0xEE, sizeof L.out);
                memset(dtile.data(), 0xEE, dtile.size());
                if (tiled) tiled_tile(J, k, c0, r0, wide, L);
                else direct_tile(J, k, c0, r0, wide, (uint8_t (*)[HVQ_SC_DTW])dtile.data());
                for (uint32_t row = r0; row < std::min(r0 + th, J.my); ++row)        /* every dword of the tile inside the plane: one store */
                    for (uint32_t col = c0; col < std::min(c0 + tw, J.mx); col += 4u) {
                        uint8_t *d = (uint8_t *)fake_span((const void *)(uintptr_t)(J.dst + (uint64_t)row * J.mx + col), 4, "scale: a dword of the target plane");
                        memcpy(d, tiled ? &L.out[row - r0][col - c0] : &dtile[(size_t)(row - r0) * HVQ_SC_DTW + (col - c0)], 4);
                        for (uint32_t i = 0; i < 4u; ++i) ++stored[(size_t)row * J.mx + col + i];
                    }
            }
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] != 1) fake_die("scale: job %d: target sample %zu was stored %u times", k, i, stored[i]);
        }
    });
}
