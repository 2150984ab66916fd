/*
 * tests/native/fake_phash.cpp -- TEST INFRASTRUCTURE: the CPU bodies of hvq_launch_hashes and hvq_launch_hash_nearest
 * (hvqm4_amd/csrc/hvq_phash.hip) for the CPU fake device.  Linked into the hash driver only (tests/test_phash_cpu.py); the other drivers link
 * without it, and the runtime's weak references then make hvq_picture_hashes and hvq_hash_nearest refuse.
 *
 * A launch is queued on its stream like any other operation; when its body runs it walks the grid the way hvq_phash_cells_kernel does
 * (pictures x workgroups, a workgroup one row cell and one chunk of column units), reaches every byte through fake_span at that moment,
 * ADDS into the picture's cells as the kernel's atomics do -- cells that were not zeroed in front of the launch show in the values -- and
 * then writes every record from the cells as hvq_phash_finish_kernel does (hvq_phash_record of hvq_phash.h).
 */
#include "fake_device.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_phash.h"

extern "C" hipError_t hvq_launch_hashes(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    if (njobs > 65535 || !max_wgs) return hipErrorInvalidValue;                   /* hvq_launch_hashes: one grid row per picture */
    return fake_enqueue(stream, "hashes", [=]() {
        const HvqHashJob *jobs = (const HvqHashJob *)fake_span(jobs_dev, (size_t)njobs * sizeof(HvqHashJob), "hashes: the job records");
        for (int k = 0; k < njobs; ++k) {
            const HvqHashJob &J = jobs[k];
            if (J.a & 15u) fake_die("hashes: job %d: the picture is not 16-byte aligned (the kernel loads 16-byte units)", k);
            if ((J.out | J.acc) & 7u) fake_die("hashes: job %d: the record or the cells are not 8-byte aligned (64-bit atomics and stores)", k);
            if (!J.w || !J.h || (J.w & 7u) || (J.h & 7u) || J.w > HVQ_PH_MAX_SIDE || J.h > HVQ_PH_MAX_SIDE) fake_die("hashes: job %d: %u x %u", k, J.w, J.h);
            const uint32_t nc = (J.w & 8u) ? 8u : 16u;
            const uint32_t cpw = J.cells_pw;
            if ((cpw != 1u && cpw != 2u && cpw != 4u && cpw != 8u) || cpw > HVQ_PH_MAX_CPW || (HVQ_PH_LANES >> J.sub_shift) != cpw)
                fake_die("hashes: job %d: %u row cells a workgroup, lanes of one 2^%u", k, cpw, J.sub_shift);
            if (J.units * nc != J.w || J.lanes_x != std::min(J.units, HVQ_PH_LANES) || J.rows_pp != (HVQ_PH_LANES / cpw) / J.lanes_x || !J.rows_pp ||
                J.wgs != HVQ_PH_ROWS / cpw * ((J.units + HVQ_PH_LANES - 1u) / HVQ_PH_LANES))
                fake_die("hashes: job %d: units %u, lanes_x %u, rows_pp %u, wgs %u do not describe a row of %u samples", k, J.units, J.lanes_x, J.rows_pp, J.wgs, J.w);
            if (J.wgs > max_wgs) fake_die("hashes: job %d needs %u workgroups, the grid has %u per picture", k, J.wgs, max_wgs);
            uint64_t *acc = (uint64_t *)fake_span((const void *)(uintptr_t)J.acc, HVQ_PH_CELLS * 8u, "hashes: a picture's cells");
            for (uint32_t wg = 0; wg < max_wgs; ++wg) {
                if (wg >= J.wgs) break;                                          /* hvq_phash_cells_kernel: workgroups past the picture leave */
                const uint32_t groups = HVQ_PH_ROWS / cpw, xc = wg / groups, r0 = (wg - xc * groups) * cpw;
                for (uint32_t r = r0; r < r0 + cpw; ++r) {                        /* the workgroup's row cells, one group of lanes each */
                const uint32_t u0 = xc * HVQ_PH_LANES, u1 = std::min(J.units, u0 + HVQ_PH_LANES);
                const uint32_t x0 = u0 * nc, x1 = u1 * nc;                       /* the workgroup's columns */
                uint64_t cells[HVQ_PH_COLS] = { 0 };
                for (uint32_t y = hvq_ph_first(32u, J.h, r); y < hvq_ph_end(32u, J.h, r); ++y) {
                    const uint32_t wy = hvq_ph_weight(32u, J.h, r, y);
                    if (!wy) fake_die("hashes: job %d: row %u has no share in row cell %u", k, y, r);
                    const uint8_t *row = (const uint8_t *)fake_span((const void *)(uintptr_t)(J.a + (size_t)y * J.w + x0), x1 - x0, "hashes: a workgroup's samples of a row");
                    for (uint32_t x = x0; x < x1; ++x) {
                        const uint64_t v = (uint64_t)wy * row[x - x0];
                        /* the cells sample x has a share in: from floor(g x / w) on, while the weight is positive */
                        for (uint32_t c = 32u * x / J.w; c < 32u && hvq_ph_weight(32u, J.w, c, x); ++c) cells[c] += v * hvq_ph_weight(32u, J.w, c, x);
                        for (uint32_t c = 9u * x / J.w; c < 9u && hvq_ph_weight(9u, J.w, c, x); ++c) cells[32u + c] += v * hvq_ph_weight(9u, J.w, c, x);
                    }
                }
                for (uint32_t c = 0; c < HVQ_PH_COLS; ++c) acc[r * HVQ_PH_COLS + c] += cells[c];
                }
            }
        }
        /* hvq_phash_finish_kernel, behind every workgroup of the first launch */
        for (int k = 0; k < njobs; ++k) {
            const HvqHashJob &J = jobs[k];
            const uint64_t *acc = (const uint64_t *)fake_span((const void *)(uintptr_t)J.acc, HVQ_PH_CELLS * 8u, "hashes: a picture's cells");
            uint64_t *out = (uint64_t *)fake_span((const void *)(uintptr_t)J.out, 32, "hashes: an output record");
            /* the weights of a sample add up to 32 x 32 in one grid and to 32 x 9 in the other: both grids hold the same sum of samples */
            uint64_t s32 = 0, s9 = 0;
            for (uint32_t r = 0; r < HVQ_PH_ROWS; ++r)
                for (uint32_t c = 0; c < HVQ_PH_COLS; ++c) (c < 32u ? s32 : s9) += acc[r * HVQ_PH_COLS + c];
            if (s32 * 9u != s9 * 32u)
                fake_die("hashes: job %d: the two grids do not hold the same picture (%llu, %llu)", k, (unsigned long long)s32, (unsigned long long)s9);
            uint64_t rec[4];
            hvq_phash_record(acc, (uint64_t)J.w * J.h, rec);
            for (int v = 0; v < 4; ++v) out[v] = rec[v];
        }
    });
}

extern "C" hipError_t hvq_launch_hash_nearest(const uint64_t *q, uint32_t nq, uint32_t q_stride, const uint64_t *db, uint32_t ndb, uint32_t db_stride,
                                              int64_t self_offset, uint32_t threshold, int32_t *out, hipStream_t stream)
{
    if (!nq) return hipSuccess;
    if (nq > HVQ_HN_MAX || ndb > HVQ_HN_MAX || threshold > 64u || !q_stride || !db_stride) return hipErrorInvalidValue;
    return fake_enqueue(stream, "hash_nearest", [=]() {
        if (((uintptr_t)q | (uintptr_t)db) & 7u) fake_die("hash_nearest: q or db is not 8-byte aligned");
        if ((uintptr_t)out & 15u) fake_die("hash_nearest: out is not 16-byte aligned (one 16-byte store per record)");
        /* workgroup by workgroup, a lane a query: the records of a workgroup are computed before any of them is stored */
        for (uint32_t i0 = 0; i0 < nq; i0 += HVQ_HN_LANES) {
            const uint32_t cnt = std::min(nq - i0, HVQ_HN_LANES);
            int32_t rec[HVQ_HN_LANES][4];
            for (uint32_t l = 0; l < cnt; ++l) {
                const uint32_t i = i0 + l;
                const uint64_t qi = *(const uint64_t *)fake_span(q + (size_t)i * q_stride, 8, "hash_nearest: a query");
                const uint32_t lim = self_offset < 0 ? ndb : (uint32_t)std::min<int64_t>((int64_t)ndb, self_offset + (int64_t)i);
                uint32_t key = (65u << 24) | 0xFFFFFFu, within = 0;
                int32_t first = -1;
                for (uint32_t j = 0; j < lim; ++j) {
                    const uint64_t x = qi ^ *(const uint64_t *)fake_span(db + (size_t)j * db_stride, 8, "hash_nearest: a database hash");
                    const uint32_t d = (uint32_t)__builtin_popcountll(x);
                    key = std::min(key, (d << 24) | j);
                    if (d <= threshold) { ++within; if (first < 0) first = (int32_t)j; }
                }
                rec[l][0] = lim ? (int32_t)(key & 0xFFFFFFu) : -1;
                rec[l][1] = lim ? (int32_t)(key >> 24) : 65;
                rec[l][2] = (int32_t)within;
                rec[l][3] = first;
            }
            int32_t *o = (int32_t *)fake_span(out + (size_t)i0 * 4u, (size_t)cnt * 16u, "hash_nearest: the records of a workgroup");
            for (uint32_t l = 0; l < cnt; ++l)
                for (int v = 0; v < 4; ++v) o[l * 4u + (uint32_t)v] = rec[l][v];
        }
    });
}
