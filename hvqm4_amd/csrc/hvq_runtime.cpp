/*
 * hvq_runtime.cpp -- host side of the MI355X HVQM4 back end: the C ABI of include/hvqm4.h
 * (the reference's SDK entry points, h4m_audio_decode.c:275, 819, 828, 957, 1970, 2018, 2058)
 * and include/hvqm4_amd.h (batched device-resident path).
 *
 * Picture-buffer rotation of the reference player (h4m:2087-2093, 2131-2137) is restated as
 * slot assignment: every decoded picture gets a slot in an HBM-resident ring of its stream,
 * anchors (I/P) stay pinned while they are the past/future reference.  Queued pictures are
 * grouped into dependency LEVELS (RAW on reference slots, WAR/WAW on the destination slot);
 * one kernel launch reconstructs one level across all streams.  Workgroups are dealt to the
 * tile table so that all tiles of a picture land on one XCD (blockIdx % 8), keeping its map,
 * nest and reference-picture reads in that XCD's L2.
 *
 * There is NO CPU reconstruction path: without a usable HIP device every entry point that
 * would produce pixels fails with HVQ_E_NOGPU.
 */
#include <hip/hip_runtime.h>
#if defined(__x86_64__)
#include <emmintrin.h>
#endif

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <thread>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/hvqm4.h"
#include "../../include/hvqm4_amd.h"
#include "hvq_desc.h"
#include "hvq_parse.h"
#include "hvq_gparse_core.h"
#include "hvq_checksum.h"
#include "hvq_jpeg.h"
#include "hvq_phash.h"
#include "hvq_scale.h"
#include "hvq_filter.h"
#include "hvq_rank.h"
#include "hvq_bilateral.h"
#include "hvq_map.h"
#include "hvq_label.h"
#include "hvq_corner.h"
#include "hvq_distance.h"
#include "hvq_integral.h"
#include "hvq_warp.h"
#include "hvq_compose.h"

#ifdef GP_PROBE
extern "C" hipError_t hvq_launch_parse_probe(const HvqParseJob *jobs_dev, HvqParseResult *results_dev, uint32_t n, uint32_t rowbuf_stride,
                                             uint32_t exit_at, hipStream_t stream);
#endif
extern "C" hipError_t hvq_launch_parse(const HvqParseJob *jobs_dev, HvqParseResult *results_dev, uint32_t n,
                                       uint32_t rowbuf_stride, uint32_t use_flat, const uint32_t *redo_dev, uint64_t *timing_dev,
                                       hipStream_t stream);
extern "C" hipError_t hvq_launch_nest_commit(const uint64_t *pairs_dev, uint32_t n, hipStream_t stream);
extern "C" uint32_t hvq_gparse_scratch_bytes(uint32_t total_blocks, uint32_t total_runs, uint32_t nmb);
extern "C" int hvq_parse_occupancy(uint32_t rowbuf_stride);

extern "C" hipError_t hvq_launch_recon_inline(const HvqJob *jobs_dev, uint32_t nslots, uint32_t max_wgs, uint32_t tiles_per_wg,
                                              uint32_t items_cap, uint32_t pair_cap, uint32_t pool_cap, hipStream_t stream);
extern "C" uint32_t hvq_recon_inline_static_lds(uint32_t tiles_per_wg, uint32_t items_cap);
extern "C" uint32_t hvq_recon_inline_dyn_lds(uint32_t pair_cap, uint32_t pool_cap);
extern "C" uint32_t hvq_recon_inline_max_wgs(uint32_t tiles_per_wg, uint32_t items_cap);
extern "C" hipError_t hvq_launch_gather(const uint64_t *src_dev, uint8_t *dst_dev, uint32_t n, uint32_t pic_bytes, hipStream_t stream);
extern "C" hipError_t hvq_launch_upload(const void *src_pinned, void *dst_dev, size_t bytes, hipStream_t stream);
extern "C" hipError_t hvq_launch_selfref(const HvqJob *job_dev, const uint8_t *side, uint8_t *dst, hipStream_t stream);
extern "C" hipError_t hvq_launch_table_div(uint32_t *out_dev, hipStream_t stream);

#ifdef HVQ_STAMPS
extern "C" void hvq_set_stamps(unsigned long long *p);
#endif
extern "C" hipError_t hvq_launch_rgb(const void *jobs_dev, int njobs, int max_lanes, int wide, int format, hipStream_t stream);
extern "C" hipError_t hvq_launch_tensor(const void *jobs_dev, int njobs, int max_lanes, int dtype, const HvqTensorNorm *nm, hipStream_t stream);
extern "C" hipError_t hvq_launch_resample(const void *jobs_dev, int njobs, int max_wgs, int dtype, const HvqTensorNorm *nm, hipStream_t stream);
/* hvq_metrics.hip.  Weak: a build of the runtime without that unit links, and hvq_picture_metrics then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_metrics(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream);
/* hvq_ssim.hip.  Weak for the same reason: hvq_picture_ssim then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_ssim(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream);
/* hvq_checksum.hip.  Weak for the same reason: hvq_picture_checksums then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_checksums(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream);
/* hvq_histogram.hip.  Weak for the same reason: hvq_picture_histograms then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_histograms(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream);
/* hvq_motion.hip.  Weak for the same reason: hvq_picture_motion then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_motion(const void *jobs_dev, int njobs, uint32_t max_tiles, int block, int radius, hipStream_t stream);
/* hvq_jpeg.hip.  Weak for the same reason: hvq_encode_jpeg then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_jpeg(const void *jobs_dev, int njobs, uint32_t max_mh, uint32_t quant_off, void *scratch, hipStream_t stream);
/* hvq_phash.hip.  Weak for the same reason: hvq_picture_hashes and hvq_hash_nearest then refuse with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_hashes(const void *jobs_dev, int njobs, uint32_t max_wgs, hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t hvq_launch_hash_nearest(const uint64_t *q, uint32_t nq, uint32_t q_stride, const uint64_t *db, uint32_t ndb, uint32_t db_stride,
                                                                    int64_t self_offset, uint32_t threshold, int32_t *out, hipStream_t stream);

/* hvq_scale.hip.  Weak for the same reason: hvq_scale_pictures then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_scale(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
/* hvq_filter.hip.  Weak for the same reason: hvq_filter_pictures then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_filter(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
/* hvq_rank.hip.  Weak for the same reason: hvq_rank_pictures then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_rank(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
/* hvq_bilateral.hip.  Weak for the same reason: hvq_bilateral_pictures then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_bilateral(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
/* hvq_map.hip.  Weak for the same reason: hvq_map_pictures and hvq_histogram_tables then refuse with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_map(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t hvq_launch_tables(const void *jobs_dev, int nrecords, hipStream_t stream);
/* hvq_label.hip.  Weak for the same reason: hvq_label_pictures and hvq_select_components then refuse with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_label(const void *jobs_dev, int npics, uint32_t max_tiles, uint32_t max_seams, uint32_t max_chunks,
                                                             hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t hvq_launch_select(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
/* hvq_corner.hip.  Weak for the same reason: hvq_corner_pictures then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_corner(const void *jobs_dev, int npics, uint32_t max_tiles, uint32_t max_rows, hipStream_t stream);
/* hvq_distance.hip.  Weak for the same reason: hvq_distance_pictures and hvq_distance_mask then refuse with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_distance(const void *jobs_dev, int npics, uint32_t max_colgroups, uint32_t max_rowgroups, hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t hvq_launch_distance_mask(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
/* hvq_integral.hip.  Weak for the same reason: hvq_integral_pictures, hvq_window_pictures and hvq_rect_sums then refuse with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_integral(const void *jobs_dev, int npics, uint32_t max_rowgroups, uint32_t max_colgroups, hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t hvq_launch_window(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t hvq_launch_rects(const void *head_dev, int npics, uint32_t nrects, hipStream_t stream);
/* hvq_warp.hip.  Weak for the same reason: hvq_warp_pictures then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_warp(const void *jobs_dev, int npics, uint32_t max_tiles, hipStream_t stream);
/* hvq_compose.hip.  Weak for the same reason: hvq_compose_pictures then refuses with HVQ_E_NOGPU */
extern "C" __attribute__((weak)) hipError_t hvq_launch_compose(const void *tab_dev, int ntargets, uint32_t max_tiles, hipStream_t stream);

#define HVQ_EXPORT extern "C" __attribute__((visibility("default")))

/* Reuse window a launch group may span (hvq_launch_group_plan, hvq_context_set_group_bytes), bytes: 512 MiB.  A window counts every
 * P/B picture twice (written once, reading as much), so this is about 256 MiB of distinct lines, the last-level cache.  The dense
 * benchmark batch (128 streams of 640x480, window 707.8 MB) runs as two groups, which is what the sweep found best (one group 0.917,
 * two 0.895, three 0.955, four 0.903, six 1.044 ms per step: profiles/r10_launch_groups.txt); BASELINE config 4 (221.2 MB) and
 * everything smaller stay one group. */
#define HVQ_GROUP_BYTES_DEFAULT (512ull << 20)

/* ---- LDS sizing of one launch of hvq_recon_inline_kernel (pure apart from the two environment caps HVQM4_AMD_PAIR_CAP and
 * HVQM4_AMD_POOL_CAP, read once per process: hvq_flush_end calls it per launch, tests/test_recon_plan.py directly) ----
 * The kernel keeps its item queue, pair list and the tile range of the pool in LDS: accumulator rows and a block column for the items of
 * the launch's fullest tile (x tiles per workgroup), a pair list for its pairs, the staged pool for its bases, scalars and a few literal
 * blocks.  A CU has 160 KB of LDS and takes 8 workgroups of 4 waves; the two-tile kernels with accumulators for 128 items and more are
 * allocated for 7 (hvq_kernels.hip, InlWaves). */
static const uint32_t HVQ_CU_LDS = 163840u;
static const uint32_t HVQ_LIT_RESERVE = 128u;            /* staged-pool dwords per tile kept for literal blocks (4 dwords each) */

HVQ_EXPORT uint32_t hvq_recon_inline_residency(uint32_t tpw, uint32_t items_cap, uint32_t lds_bytes)
{
    return std::min(hvq_recon_inline_max_wgs(tpw, items_cap), HVQ_CU_LDS / std::max(lds_bytes, 1u));
}

/* the shape of a launch with `t` tiles per workgroup whose fullest tile has `mi` items and `mp` pairs */
static uint32_t inline_sized(uint32_t t, uint32_t mi, uint32_t mp, uint32_t *cap, uint32_t *pairs, uint32_t *pool)
{
    /* the kernel's instantiations (hvq_launch_recon_inline); 64 is the least: a wave's blocks pass through its accumulators on their way out */
    static const uint32_t steps2[] = { 64, 96, 128, 160, 192, 224, 256, 384, 512 }, steps1[] = { 64, 96, 128, 192, 256 };
    /* more pairs than the list holds: the items walk their bases (HVQM4_AMD_PAIR_CAP, tests: ordinary clips reach that path) */
    static const uint32_t pair_lim = getenv("HVQM4_AMD_PAIR_CAP") ? (uint32_t)std::max(1, atoi(getenv("HVQM4_AMD_PAIR_CAP"))) : 4096u;
    /* HVQM4_AMD_POOL_CAP (tests): a smaller staging area, so that ordinary clips reach the read-from-HBM path of tiles
     * whose payload exceeds it */
    static const uint32_t pool_lim = getenv("HVQM4_AMD_POOL_CAP") ? (uint32_t)std::max(0, atoi(getenv("HVQM4_AMD_POOL_CAP"))) : 1536u;
    const uint32_t want = std::min(256u * t, std::max(64u, t * mi));
    uint32_t ic = t == 2 ? 512u : 256u;
    for (uint32_t v : steps2) if (t == 2 && v >= want) { ic = v; break; }
    for (uint32_t v : steps1) if (t == 1 && v >= want) { ic = v; break; }
    *cap = ic;
    *pairs = std::max(1u, std::min(pair_lim, t * mp));
    *pool = std::min(pool_lim, t * (mp + 2u * mi + HVQ_LIT_RESERVE));
    const uint32_t reserve = *pool - std::min(*pool, t * (mp + 2u * mi));      /* what the limit left of the literal reserve */
    if (*pool) *pool = (*pool + 4u + 3u) & ~3u;      /* + 4: the staged range starts at the 16-byte boundary below the tile's first dword */
    uint32_t bytes = hvq_recon_inline_static_lds(t, ic) + hvq_recon_inline_dyn_lds(*pairs, *pool);
    /* A launch that misses the next residency step by no more than the literal reserve its pool holds gives that much of it up -- never
     * room for bases and scalars: a pool the limit has clipped below them has no reserve and is not trimmed.  Only the staged pool is
     * ever trimmed: it is the one part that overflows gracefully (payload beyond it is read from HBM); a short pair list turns the tile
     * serial, items beyond the cap are dropped. */
    const uint32_t res = hvq_recon_inline_residency(t, ic, (bytes + 511u) & ~511u);
    if (res < hvq_recon_inline_residency(t, ic, 1u)) {
        const uint32_t target = HVQ_CU_LDS / (res + 1u) & ~511u;
        const uint32_t cut = bytes > target ? (bytes - target + 15u) / 16u * 4u : 0u;      /* dwords, in the pool's 16-byte pieces */
        if (cut && cut <= reserve) {
            *pool -= cut;
            bytes = hvq_recon_inline_static_lds(t, ic) + hvq_recon_inline_dyn_lds(*pairs, *pool);
        }
    }
    return (bytes + 511u) & ~511u;
}

/* One or two tiles per workgroup, and the launch's LDS shape.  force_tpw: 0 = decide here, 1 / 2 = that many (HVQM4_AMD_TILES_PER_WG).
 * lds_bytes: static + dynamic LDS of the launch, rounded up to 512. */
HVQ_EXPORT void hvq_recon_inline_plan(uint32_t max_items, uint32_t max_pairs, int force_tpw, uint32_t *tpw, uint32_t *items_cap,
                                      uint32_t *pair_cap, uint32_t *pool_cap, uint32_t *lds_bytes)
{
    uint32_t cap1, pr1, po1, cap2, pr2, po2;
    const uint32_t lds1 = inline_sized(1, max_items, max_pairs, &cap1, &pr1, &po1), lds2 = inline_sized(2, max_items, max_pairs, &cap2, &pr2, &po2);
    const uint32_t tiles1 = hvq_recon_inline_residency(1, cap1, lds1), tiles2 = 2u * hvq_recon_inline_residency(2, cap2, lds2);
    /* Two tiles per workgroup when they keep at least 1.5 times the tiles of the one-tile launch resident.  Measured on the dense stream
     * (profiles/r07_two_tiles_dense.txt, one box, three runs each, ms per step): two tiles at seven workgroups per CU 0.919, at six
     * (HVQM4_AMD_LDS_PAD) 0.925, one tile at eight 0.929 -- six still wins by less than the spread of a run (0.5 %), so the rule stays
     * where round 4 put it (sparse streams: 16 tiles against 8) and a launch whose fullest tile needs accumulators for 192 items keeps
     * its two tiles at six. */
    const bool two = lds2 <= 65536u && (force_tpw ? force_tpw >= 2 : 2u * tiles2 >= 3u * tiles1);
    *tpw = two ? 2u : 1u;
    *items_cap = two ? cap2 : cap1; *pair_cap = two ? pr2 : pr1; *pool_cap = two ? po2 : po1;
    *lds_bytes = two ? lds2 : lds1;
}

/* Launch groups of a batch (build_tiles): into how many groups of streams its launches are split, and which stream goes where.  Pure;
 * it sees what build_tiles knows at begin -- per stream its picture size and the kinds and levels of its pending pictures (pictures
 * [first[s], first[s + 1]) of `kinds` / `levels`; HVQ_PIC_*), no blob lengths.
 *   A stream's reuse window is the largest sum, over two consecutive levels, of the algorithmic bytes of its pictures in them (written
 *   once, P/B pictures read as much again): what is touched between an anchor's write and its last read one level later.  The batch's
 *   window is the sum over its streams, G = ceil(window / budget) -- at most so many that every group keeps 8 streams per launch queue
 *   (the 8 picture slots that spread a launch over the XCDs); budget 0, or a window within it: 1.
 *   Streams go to the groups by work (algorithmic bytes of all their pictures), heaviest first to the lightest group that is not full: a
 *   group is full at floor(n / G) streams, n % G groups take one more, so no group falls below the minimum.
 * group_of (nstreams entries) and window may be null.  Returns G >= 1. */
HVQ_EXPORT uint32_t hvq_launch_group_plan(uint32_t nstreams, const uint32_t *pic_bytes, const uint32_t *first, const uint8_t *kinds,
                                          const int32_t *levels, uint64_t budget, uint32_t queues, uint16_t *group_of, uint64_t *window)
{
    std::vector<uint64_t> work(nstreams, 0), per_level;
    uint64_t win = 0;
    for (uint32_t s = 0; s < nstreams; ++s) {
        per_level.clear();
        for (uint32_t i = first[s]; i < first[s + 1]; ++i) {
            const size_t l = (size_t)std::max(levels[i], 0);
            if (per_level.size() < l + 2) per_level.resize(l + 2, 0);
            const uint64_t b = (uint64_t)pic_bytes[s] * (kinds[i] == HVQ_PIC_I ? 1u : 2u);
            per_level[l] += b; work[s] += b;
        }
        uint64_t w = 0;
        for (size_t l = 0; l + 1 < per_level.size(); ++l) w = std::max(w, per_level[l] + per_level[l + 1]);
        win += w;
    }
    if (window) *window = win;
    const uint32_t min_streams = 8u * std::max(queues, 1u);
    uint64_t g64 = budget ? (win + budget - 1) / budget : 1;
    g64 = std::min<uint64_t>(g64, nstreams / min_streams);
    const uint32_t G = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(g64, 1), 65535);
    if (!group_of) return G;
    std::vector<uint32_t> order(nstreams);
    for (uint32_t s = 0; s < nstreams; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return work[a] > work[b]; });
    std::vector<uint64_t> load(G, 0);
    std::vector<uint32_t> count(G, 0);
    const uint32_t base = nstreams / G;
    uint32_t extra = nstreams % G;                     /* groups that may still take one stream more than `base` */
    for (uint32_t s : order) {
        uint32_t g = G;
        for (uint32_t k = 0; k < G; ++k) {
            if (count[k] > base || (count[k] == base && !extra)) continue;
            if (g == G || load[k] < load[g]) g = k;
        }
        if (count[g] == base) --extra;
        group_of[s] = (uint16_t)g; load[g] += work[s]; ++count[g];
    }
    return G;
}

/* the budget a new context carries (hvq_context_set_group_bytes changes it) */
HVQ_EXPORT uint64_t hvq_launch_group_default_bytes(void) { return HVQ_GROUP_BYTES_DEFAULT; }

static thread_local std::string g_err;
static thread_local int g_sdk_err = 0;

static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(HVQ_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

HVQ_EXPORT const char *hvq_last_error_string(void) { return g_err.c_str(); }

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* workgroups of a picture: one per pair of consecutive tiles of a plane (the kernel's mapping) */
static uint32_t picture_workgroups(const uint32_t tile_first[4])
{
    uint32_t n = 0;
    for (int k = 0; k < 3; ++k) n += (tile_first[k + 1] - tile_first[k] + 1) / 2;
    return n;
}

/* Pictures this back end refuses instead of decoding them differently from the reference:
 *   HVQ_F_CAPPED    an overflow-symbol run ended on the parsers' cap: the reference would have gone on summing (h4m:654-677);
 *   HVQ_F_CLAMPED   a nest origin or vector target outside what the reference's arithmetic keeps in bounds was clamped, or the
 *                   picture reads outside the referenced picture or from an empty section (hvq_refuse.h; malformed input);
 *                   HVQM4_AMD_ALLOW_CLAMPED=1 decodes such pictures with clamped addresses;
 *   HVQ_F_MALFORMED a P/B luma kind symbol above 15, or a type run that opens at value 3: the reference decodes those outside its own
 *                   rules (stored type / proc bits, a table index and a residual-bit count the stream does not set); or a prefix tree
 *                   with more inner nodes than 256 leaf bytes allow (the GPU parser rejects it too).  Not opt-in. */
static const char *unsupported_reason(uint32_t flags)
{
    if (flags & HVQ_F_CAPPED) return "an overflow-symbol run is longer than this back end follows (the reference sums for as long as the stream says, h4m:654-677)";
    if (flags & HVQ_F_MALFORMED) return "malformed picture: a P/B luma kind symbol above 15 (h4m:1701, 1927), a macroblock type run that opens at value 3 (h4m:1591, 1606, 1950-1951) or a prefix tree with more inner nodes than 256 leaves allow";
    if (flags & HVQ_F_CLAMPED) {
        const char *e = getenv("HVQM4_AMD_ALLOW_CLAMPED");
        if (!(e && atoi(e) > 0)) return "malformed picture: a nest origin or vector target had to be clamped, a motion-compensated block or window basis reads outside the referenced picture, or an empty section is read (HVQM4_AMD_ALLOW_CLAMPED=1 decodes it anyway)";
    }
    return nullptr;
}

/* ------------------------------------------------------------------ context */
struct Slot {
    int w_level = -1;   /* level (in the pending batch) of the launch that writes the current content */
    int r_level = -1;   /* highest level that reads it */
    int pic = -1;       /* ordinal of the occupant */
};

struct Stream {
    bool open = false;
    HvqParser *parser = nullptr;
    int w = 0, h = 0;
    int wshift = 0, hshift = 0;              /* chroma subsampling (hvq_parser_create) */
    uint32_t pic_bytes = 0, slot_bytes = 0;
    uint8_t *dev = nullptr;                  /* (nslots + 1) slots; the last one stays zero */
    std::vector<Slot> slots;
    int anchor_old = -1, anchor_new = -1;    /* "past" / "future" of the reference player */
    int ring = 0;
    int npics = 0;
    std::vector<int> pic_slot;
    /* GPU entropy parse (hvq_submit_many_device): the stream's pictures never meet the host parser */
    int parse_mode = 0;                      /* 0 undecided, 1 host parser, 2 device parser */
    HvqPicHeader layout{};                   /* geometry part of every blob of this stream */
    uint32_t blob_cap = 0, scratch_bytes = 0;
    uint8_t *nest_keep = nullptr;            /* two slots: [nest_cur] = packed nest of the last I picture of earlier
                                                batches (zero before any); a flush commits into the other slot */
    int nest_cur = 0;
    uint8_t *nest_keep_ptr(int which) const { return nest_keep + (size_t)which * GP_ALIGN16(HVQ_NESTP_BYTES); }
    int nest_src = -1;                       /* pending index of the last I picture queued in this batch, -1: nest_keep */
    bool need_I = false;                     /* a picture of this stream was rejected: P/B pictures are refused until the next I picture */
    /* the reference player's three buffers (h4m:2087-2093, 2131-2137), as ordinals of the pictures they hold (-1: never written):
     * a P picture with future-referencing macroblocks reads what `present` held before (h4m:2058-2061) */
    int rp_past = -1, rp_future = -1, rp_present = -1;
    const void *sdk_present = nullptr;       /* SDK path: the caller's `present` buffer of the picture being submitted */
    int inflight_from = 0x7FFFFFFF;          /* ordinals >= this belong to the batch between hvq_flush_begin and hvq_flush_end */
    uint8_t *slot_ptr(int s) const { return dev + (size_t)(s < 0 ? (int)slots.size() : s) * slot_bytes; }
};

struct Pending {
    uint32_t max_items, max_pairs;
    int stream, ordinal, level;
    size_t blob_off, blob_len;
    int dst, ref0, ref1;
    uint32_t ntiles, kind;
    uint32_t nwg;                      /* workgroups: pairs of consecutive tiles, plane by plane */
    uint32_t w, h;
    /* device-parsed pictures: raw bitstream in the arena instead of a blob */
    bool dev = false;
    int nest_ref = -1;                 /* pending index of the governing I picture, -1: the stream's nest_keep */
    uint64_t dev_blob = 0, dev_nest = 0, nest_ptr = 0;
    uint32_t flags = 0, unk_shift = 0, pool_dwords = 0;
    int status = 0;                    /* device parse status bits (GP_ST_*) */
    bool redo = false;                 /* GPU-parsed picture whose overflow run outlasted the device parser's cap: parsed again on the host,
                                          its blob lies at rp_dev + redo_off, its header in redo_hd */
    size_t redo_off = 0;
    HvqPicHeader redo_hd{};
    bool dropped = false;              /* rejected at flush time (or follows a rejected picture of its stream): not reconstructed */
    int old_slot = -1;                 /* P pictures: slot that holds what the reference's `present` buffer held before this picture
                                          (-1: never written -> the zero slot; -2: that picture's slot has been reused since) */
    const void *host_old = nullptr;    /* SDK path: the caller's `present` buffer itself */
};

struct Launch {
    int level;
    int queue;                         /* launch queue (0: the main stream, 1: stream2) */
    int group;                         /* launch group of its streams (build_tiles): a queue runs group 0's levels, then group 1's, ... */
    uint32_t first_tile, ntiles;       /* its picture slots in the launch table: first entry, count */
    uint32_t max_tiles, workgroups;    /* grid = (8, max_tiles, slots / 8) at the chosen tiles per workgroup; workgroups that do work */
    uint32_t max_wg[2], wgs[2];        /* the same for one / two tiles per workgroup (chosen at flush_end, when the queues are known) */
    uint32_t tpw;
    uint32_t items_cap;                /* LDS sizing of the launch: max over its pictures */
    uint32_t pair_cap, pool_cap;       /* its dynamic LDS: pair list entries, staged pool dwords */
};

/* a P picture with future-referencing macroblocks, behind the launch of its level: previous content into the destination slot
 * (unless it is there already), then the raster-order walk (hvq_selfref_kernel) from the side buffer */
struct SelfRef {
    int launch;                        /* the launch of its picture's group, level and queue (index into `launches`) */
    uint32_t job;                      /* launch slot */
    const uint8_t *old_dev;            /* device source of the previous content, nullptr: in place already */
    const void *old_host;              /* SDK path: host source */
    uint8_t *dst;
    size_t side_off;                   /* side buffer inside selfref_dev */
    uint32_t pic_bytes;
};

struct HvqContext {
    int device = 0;
    hipStream_t stream = nullptr;      /* every launch of a batch: its dependency levels in order */
    hipStream_t qstream[4] = { nullptr, nullptr, nullptr, nullptr };   /* launch queues 1..3 (created on first use; queue 0 is `stream`), see build_tiles */
    hipEvent_t ev_fork = nullptr, ev_join[4] = { nullptr, nullptr, nullptr, nullptr };
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<Stream> streams;
    /* staging: pinned host arena mirrored by a device arena */
    uint8_t *host_arena = nullptr, *dev_arena = nullptr;
    size_t arena_cap = 0, arena_used = 0;
    size_t arena_uploaded = 0;         /* [0, arena_uploaded) is already on its way to dev_arena (early H2D of bitstreams) */
    /* Two arenas: host_arena/dev_arena is the one being FILLED; the other belongs to the batch in flight (between
     * hvq_flush_begin and hvq_flush_end) or is idle.  Uploads run on their own stream so that the next batch's
     * bitstreams travel while this batch is parsed and reconstructed. */
    uint8_t *host_arena_alt = nullptr, *dev_arena_alt = nullptr;
    size_t arena_cap_alt = 0;
    int arena_id = 0;                  /* which of the two the current one is */
    bool arena_waited = false;         /* copy_stream already waits for the last batch that used the current arena */
    bool arena_host_ready = false;     /* the host has waited for that batch's upload: it may write into the current arena (arena_host_wait) */
    bool resv_active = false;          /* hvq_arena_reserve: [resv_base, resv_base + resv_bytes) of the arena being filled is the caller's to write */
    size_t resv_base = 0, resv_bytes = 0;
    hipStream_t copy_stream = nullptr, read_stream = nullptr;
    hipEvent_t ev_read = nullptr;
    hipEvent_t ev_copy = nullptr, ev_arena_free[2] = { nullptr, nullptr };
    hipEvent_t ev_h2d[2] = { nullptr, nullptr };      /* per arena: its last batch's bitstreams / blobs have left the pinned arena */
    std::vector<Pending> pending;
    /* batch in flight */
    bool fl_active = false;
    std::vector<Pending> fl_pending;
    std::vector<uint64_t> fl_nest_pairs;
    std::vector<int> fl_nest_streams;  /* stream of each pair */
    uint8_t *fl_host = nullptr, *fl_dev = nullptr;
    int fl_arena_id = 0;
    /* pinned staging of the table uploads, one set per arena id: an H2D from pageable memory would block the caller
     * until the stream has drained (the parse kernel!), which is exactly what hvq_flush_begin must not do */
    struct Pinned { uint8_t *p = nullptr; size_t cap = 0; } pin[2][5];   /* [arena id][parse jobs, tiles, jobs, nest pairs, re-parsed blobs] */
    std::vector<HvqJob> jobs_host;     /* the tables are built here, then copied into the pinned staging */
    std::vector<HvqTileRef> tiles_host;
    /* last flushed batch (kept resident for hvq_replay) */
    HvqJob *jobs_dev = nullptr;        /* one job per launch slot, in launch order (padding slots: total_tiles = 0) */
    size_t jobs_cap = 0;
    uint8_t *tq_dev = nullptr;         /* self-referencing P pictures: the pool offset of every block (written by the level's launch, read by hvq_selfref_kernel) */
    size_t tq_cap = 0;
    uint8_t *rb_dev = nullptr;         /* bulk readback: pictures gathered into one buffer, then few large copies */
    size_t rb_cap = 0;
    uint64_t *rb_tab_dev = nullptr, *rb_tab_host = nullptr;   /* their slot addresses (device table, pinned staging) */
    size_t rb_tab_cap = 0;
    uint8_t *selfref_dev = nullptr;    /* side buffers of the batch's self-referencing P pictures */
    size_t selfref_cap = 0;
    std::vector<SelfRef> selfrefs;
    std::vector<Launch> launches;
    std::vector<Launch> fl_launches;   /* of the batch in flight: tile ranges known at begin, LDS sizes at end */
    int max_queues = 2;                /* hvq_context_set_launch_queues */
    std::vector<uint8_t> fl_qof;       /* launch queue of every stream in the batch in flight (two queues: dealt by work, build_tiles) */
    uint64_t group_bytes = HVQ_GROUP_BYTES_DEFAULT;    /* hvq_context_set_group_bytes: the reuse window a launch group may span, 0: never split */
    std::vector<uint16_t> fl_gof;      /* launch group of every stream in the batch in flight (hvq_launch_group_plan) */
    uint32_t fl_groups = 1, groups = 0;                /* G of the batch in flight; of the resident batch (0: none) */
    HvqStats stats{};
    double parse_seconds = 0;
    std::atomic<uint64_t> copy_bytes{ 0 };     /* bitstream bytes copied into the pinned arena (copy threads), and their wall time in ns */
    std::atomic<uint64_t> copy_ns{ 0 };
    uint8_t *rgb_dev = nullptr;        /* scratch of the display epilogue */
    size_t rgb_cap = 0;
    HvqRgbJob *rgb_jobs_dev = nullptr;
    size_t rgb_jobs_cap = 0;
    /* hvq_export_pictures / hvq_export_tensors: job tables in a ring, each reused once the export that read it has finished (its event); the newest
     * export's event orders the next export and every later slot writer (export_fence) */
    struct ExportTab { uint8_t *host = nullptr; uint8_t *dev = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; } ex[4];
    int ex_next = 0, ex_last = -1;     /* table of the next export; of the newest one (-1: none yet) */
    bool ex_unfenced = false;          /* an export was queued since c->stream last waited for one */
    /* hvq_picture_checksums: the accumulators of one call's pictures, 96 bytes each.  One buffer serves every call: a call of the export
     * chain runs behind the one before it, so the launch that zeroes and fills it comes after the launches that read it last */
    uint8_t *ck_acc = nullptr;
    size_t ck_cap = 0;
    /* hvq_encode_jpeg: per picture of one call one dword and one per restart interval (HvqJpegJob).  One buffer serves every call, as ck_acc */
    uint32_t *jp_scr = nullptr;
    size_t jp_cap = 0;                 /* dwords */
    /* hvq_picture_hashes: the cells of one launch pair's pictures, HVQ_PH_CELLS qwords each, HVQ_PH_BATCH pictures at the most.  One buffer
     * serves every launch pair and every call, as ck_acc */
    uint8_t *ph_acc = nullptr;
    size_t ph_cap = 0;
    bool cp_force_general = false;     /* hvq_compose_force_general: every layer plane takes the general body of hvq_compose.hip */
    int wp_force = 0;                  /* hvq_warp_force_direct: 0 the chosen body of hvq_warp.hip, 1 the direct one, 2 the tiled one wherever LDS holds the box */
    bool fl_force_filter = false;      /* hvq_filter_force_filter: identity planes take the filter body of hvq_filter.hip, not the copy body */
    bool rk_force_general = false;     /* hvq_rank_force_general: planes that are copied take the min/max body of hvq_rank.hip, not the copy body */
    bool bl_force_general = false;     /* hvq_bilateral_force_general: planes of radius 0 take the general body of hvq_bilateral.hip, not the copy body */
    bool sc_force_direct = false;      /* hvq_scale_force_direct: every plane takes the direct body of hvq_scale.hip */
    /* GPU entropy parse: blobs + scratch + nests of a batch, its job and result tables, the events around its parse kernel.  Two
     * sets: hvq_flush_next queues the parse of batch k + 1 BEFORE it takes the results of batch k, so the reconstruction of batch k
     * reads one set while the parse of batch k + 1 fills the other.  ps_live is the set the code below means by PS(c). */
    struct ParseSet {
        std::vector<size_t> fl_idx;        /* the batch's GPU-parsed pictures (indices into fl_pending) */
        std::vector<HvqParseJob> pjobs_host;
        HvqParseResult *pr_host = nullptr; /* pinned: the parse workgroups write their result records here */
        size_t pr_host_cap = 0;
        uint8_t *gp_dev = nullptr;
        size_t gp_cap = 0;
        HvqParseJob *pj_dev = nullptr;
        uint64_t *np_dev = nullptr;
        size_t pj_cap = 0;
        hipEvent_t ev_parse = nullptr, evp0 = nullptr, evp1 = nullptr;   /* results complete; timing of the parse kernel */
        uint32_t fl_rowbuf = 0;
        uint64_t *timing_dev = nullptr;
    } ps[2];
    int ps_live = 0;
    bool abandoned = false;                    /* flush_abandon ran since this was cleared */
    bool arena_idle[2] = { false, false };     /* nothing on the GPU reads this arena or its staging any more (hvq_flush_next) */
    double gpu_parse_ms = 0;           /* device time of the parse kernel of the last flush */
    uint32_t gpu_parse_retried = 0;    /* pictures of the last flush the flat parse path handed to the chains */
    uint32_t *redo_dev = nullptr;      /* their indices, for the chains kernel */
    uint8_t *rp_dev = nullptr;         /* blobs of the pictures parsed again on the host (overflow runs beyond the device parser's cap) */
    size_t rp_cap = 0;
    std::vector<uint8_t> rp_host;
    size_t redo_cap = 0;
    /* streaming: the bitstream copy of the batch being queued runs on a worker while the batch in flight is finished */
    std::thread copy_worker;
    bool copy_active = false;
    std::atomic<bool> copy_done{ false };      /* the worker has finished (hvq_flush_next polls it beside the parse event) */
    int copy_rc = 0;
    std::string copy_err;
};

static inline HvqContext::ParseSet &PS(HvqContext *c) { return c->ps[c->ps_live]; }
static inline const HvqContext::ParseSet &PS(const HvqContext *c) { return c->ps[c->ps_live]; }

/* Every enqueue that writes picture slots (the reconstruction and self-reference launches of a flush or replay) comes behind the
 * exports that may still read them (hvq_export_pictures, on the caller's streams): the launch stream waits for the newest export,
 * which waited for every export before it.  Ahead of queues_fork, so that both launch queues inherit the wait; nothing when no
 * export was queued since the last wait. */
static int export_fence(HvqContext *c)
{
    if (!c->ex_unfenced) return HVQ_OK;
    HIPCHK(hipStreamWaitEvent(c->stream, c->ex[c->ex_last].ev, 0));
    c->ex_unfenced = false;
    return HVQ_OK;
}

/* host side of the same before a ring is freed (hvq_stream_close, hvq_context_destroy) */
static int export_drain(HvqContext *c)
{
    if (c->ex_last >= 0) HIPCHK(hipEventSynchronize(c->ex[c->ex_last].ev));
    return HVQ_OK;
}

/* Before the HOST writes into the arena being filled: the upload of the batch that used it two flushes ago has run.  The arena is pinned
 * memory; that upload (arena_upload: copy commands on the copy stream) reads it when the GPU gets there, not when it is queued -- a caller
 * that submits and flushes small batches faster than the GPU drains them (seven clips opened, submitted and flushed back to back) used to
 * overwrite bitstreams and blobs that had not been copied yet, and the older batch was then parsed or reconstructed from the newer one's
 * bytes.  Once per arena turn, at its first write (arena_reserve: every submit path reserves before it writes); the event is the upload's
 * own (ev_h2d, begin_upload), not the end of the batch: the host copy of batch k + 1 still runs beside the reconstruction of batch k - 1.
 * hvq_flush_next knows the arena idle without asking (arena_idle) and never waits here. */
static int arena_host_wait(HvqContext *c)
{
    if (c->arena_host_ready) return HVQ_OK;
    if (!c->arena_idle[c->arena_id]) HIPCHK(hipEventSynchronize(c->ev_h2d[c->arena_id]));
    c->arena_host_ready = true;
    return HVQ_OK;
}

static int arena_reserve(HvqContext *c, size_t need)
{
    { int rcw = arena_host_wait(c); if (rcw) return rcw; }
    if (c->arena_used + need <= c->arena_cap) return HVQ_OK;
    if (c->resv_active) return fail(HVQ_E_STATE, "the arena would have to grow while a reservation of it is outstanding (hvq_submit_many_arena first)");
    size_t ncap = c->arena_cap ? c->arena_cap : (size_t)64 << 20;
    while (ncap < c->arena_used + need) ncap *= 2;
    uint8_t *nh = nullptr, *nd = nullptr;
    HIPCHK(hipHostMalloc((void **)&nh, ncap, hipHostMallocDefault));
    HIPCHK(hipMalloc((void **)&nd, ncap));
    if (c->arena_used) memcpy(nh, c->host_arena, c->arena_used);
    if (c->host_arena) {
        HIPCHK(hipStreamSynchronize(c->copy_stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipHostFree(c->host_arena));
        HIPCHK(hipFree(c->dev_arena));
    }
    c->host_arena = nh; c->dev_arena = nd; c->arena_cap = ncap;
    c->arena_uploaded = 0;             /* the new device arena holds nothing yet */
    return HVQ_OK;
}

/* queue the H2D of [arena_uploaded, upto) of the arena being filled on the copy stream */
static int arena_upload(HvqContext *c, size_t upto)
{
    if (upto <= c->arena_uploaded) return HVQ_OK;
    if (!c->arena_waited) {            /* the batch that used this arena two flushes ago may still be reconstructing */
        if (!c->arena_idle[c->arena_id]) HIPCHK(hipStreamWaitEvent(c->copy_stream, c->ev_arena_free[c->arena_id], 0));
        c->arena_waited = true;
    }
    HIPCHK(hipMemcpyAsync(c->dev_arena + c->arena_uploaded, c->host_arena + c->arena_uploaded, upto - c->arena_uploaded,
                          hipMemcpyHostToDevice, c->copy_stream));
    c->arena_uploaded = upto;
    return HVQ_OK;
}

static int flush_end(HvqContext *c);
static int flush_abandon(HvqContext *c, int rc);

/* wait for the bitstream copy of the batch being queued (hvq_submit_many_device in streaming).  A failed copy (a HIP error in one of
 * its uploads) takes the queued batch with it: its pictures were never uploaded. */
static int copy_join(HvqContext *c)
{
    if (!c->copy_active) return HVQ_OK;
    if (c->copy_worker.joinable()) c->copy_worker.join();
    c->copy_active = false;
    if (!c->copy_rc) return HVQ_OK;
    for (auto &p : c->pending) {
        Stream &s = c->streams[(size_t)p.stream];
        if ((size_t)p.ordinal < s.pic_slot.size() && s.pic_slot[(size_t)p.ordinal] == p.dst) {
            s.pic_slot[(size_t)p.ordinal] = -1;
            if (p.dst >= 0 && s.slots[(size_t)p.dst].pic == p.ordinal) s.slots[(size_t)p.dst].pic = -1;
        }
        s.anchor_old = s.anchor_new = -1; s.need_I = true; s.nest_src = -1;
    }
    c->pending.clear();
    c->arena_used = 0; c->arena_uploaded = 0;
    return fail(c->copy_rc, "bitstream upload of the queued batch failed (%s); the batch was dropped", c->copy_err.c_str());
}

/* HVQM4_AMD_FLUSH_TIMING=1: host-side timeline of the flush halves on stderr (development aid) */
static bool flush_timing() { static const bool on = getenv("HVQM4_AMD_FLUSH_TIMING") != nullptr; return on; }
static double now_ms()
{
    static const auto t0 = std::chrono::steady_clock::now();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

/* A bitstream into the pinned arena with non-temporal stores: the arena is written once and read by the DMA engine, so fetching
 * its lines into the cache first (what a plain store does) doubles the memory traffic of a copy whose 160 MB per batch have to
 * fit into the 4.7 ms the GPU takes for the batch before (HVQM4_AMD_NT_COPY=0: memcpy). */
static inline void cpu_relax()
{
#if defined(__x86_64__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

static inline void copy_to_arena(uint8_t *dst, const uint8_t *src, size_t len)
{
    static const bool nt = !(getenv("HVQM4_AMD_NT_COPY") && atoi(getenv("HVQM4_AMD_NT_COPY")) == 0);
    size_t i = 0;
#if defined(__x86_64__)
    if (nt && ((uintptr_t)dst & 15u) == 0 && len >= 4096) {
        for (; i + 64 <= len; i += 64) {
            const __m128i a = _mm_loadu_si128((const __m128i *)(src + i)), b = _mm_loadu_si128((const __m128i *)(src + i + 16)),
                          c = _mm_loadu_si128((const __m128i *)(src + i + 32)), d = _mm_loadu_si128((const __m128i *)(src + i + 48));
            _mm_stream_si128((__m128i *)(dst + i), a); _mm_stream_si128((__m128i *)(dst + i + 16), b);
            _mm_stream_si128((__m128i *)(dst + i + 32), c); _mm_stream_si128((__m128i *)(dst + i + 48), d);
        }
    }
#else
    (void)nt;
#endif
    memcpy(dst + i, src + i, len - i);
}

/* copy `bytes` into pinned staging buffer [id][which] and queue its upload to `dst` on the compute stream */
static int staged_upload(HvqContext *c, int id, int which, void *dst, const void *src, size_t bytes)
{
    HvqContext::Pinned &b = c->pin[id][which];
    if (bytes > b.cap) {
        if (b.p) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipHostFree(b.p)); b.p = nullptr; b.cap = 0; }
        const size_t ncap = align_up(bytes * 2, 4096);
        HIPCHK(hipHostMalloc((void **)&b.p, ncap, hipHostMallocDefault));
        b.cap = ncap;
    }
    memcpy(b.p, src, bytes);
    /* Tables of a few hundred KB go up by a kernel of the compute queue that reads the pinned buffer over PCIe.  A copy command goes
     * to a DMA engine, and the runtime deals engines to streams as it likes: the job table of batch k, queued at flush_end, ended up
     * behind the 160 MB of batch k + 1's bitstreams on the copy stream's engine once in four or five batches and held the
     * reconstruction -- and the parse queued behind it -- back by 1-2 ms (HVQM4_AMD_KERNEL_UPLOAD=0: copy commands).  Buffers are
     * 16-byte multiples (pinned capacity is rounded to 4 KB, device tables are allocated with slack). */
    static const bool by_kernel = !(getenv("HVQM4_AMD_KERNEL_UPLOAD") && atoi(getenv("HVQM4_AMD_KERNEL_UPLOAD")) == 0);
    if (by_kernel && bytes <= ((size_t)8 << 20) && ((uintptr_t)dst & 15u) == 0) {
        const size_t pad = align_up(bytes, 16);
        if (pad > bytes) memset(b.p + bytes, 0, pad - bytes);
        HIPCHK(hvq_launch_upload(b.p, dst, bytes, c->stream));
    } else HIPCHK(hipMemcpyAsync(dst, b.p, bytes, hipMemcpyHostToDevice, c->stream));
    return HVQ_OK;
}

HVQ_EXPORT int hvq_context_create(int device, HvqContext **out)
{
    if (!out) return fail(HVQ_E_ARG, "null out");
#if defined(__x86_64__)
    /* the host entropy parse (hvq_parse.c) is built for x86-64-v3 (csrc/Makefile) */
    if (!__builtin_cpu_supports("avx2") || !__builtin_cpu_supports("bmi2"))
        return fail(HVQ_E_ARG, "this build's host entropy parse needs an x86-64-v3 CPU (AVX2, BMI2); rebuild with HOST_ARCH= for older hosts");
#endif
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(HVQ_E_NOGPU, "no HIP device available (%s): the HVQM4 reconstruction path is GPU-only",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(HVQ_E_ARG, "device %d out of range (%d devices)", device, n);
    HIPCHK(hipSetDevice(device));
    HvqContext *c = new HvqContext();
    c->device = device;
    struct Guard { HvqContext *c; ~Guard() { if (c) hvq_context_destroy(c); } } guard{ c };     /* a failing step below frees what exists */
    {   /* The launch stream at the highest stream priority: the runtime deals a process's streams to four hardware queues in the order of
         * their creation, per priority level -- with a copy and a read-back stream per context, the launch streams of two contexts (two
         * players of one process, bench.py's two-context streaming leg) landed on ONE hardware queue and their kernels ran one after the
         * other (4.6 ms per half batch each instead of 3.6: profiles/r05_flush_next.txt 6).  At a level of their own the launch streams of
         * up to four contexts get a queue each.  HVQM4_AMD_STREAM_PRIORITY=0: plain streams as before. */
        int lo = 0, hi = 0;
        static const bool prio = !(getenv("HVQM4_AMD_STREAM_PRIORITY") && atoi(getenv("HVQM4_AMD_STREAM_PRIORITY")) == 0);
        if (prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo)
            HIPCHK(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
        else HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    }
    HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->read_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_read, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming));
    for (auto &S : c->ps) {
        HIPCHK(hipEventCreateWithFlags(&S.ev_parse, hipEventDisableTiming));
        HIPCHK(hipEventCreate(&S.evp0));
        HIPCHK(hipEventCreate(&S.evp1));
    }
    HIPCHK(hipEventCreateWithFlags(&c->ev_arena_free[0], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_arena_free[1], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_h2d[0], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_h2d[1], hipEventDisableTiming));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    guard.c = nullptr;
    *out = c;
    return HVQ_OK;
}

HVQ_EXPORT int hvq_context_set_launch_queues(HvqContext *c, int n)
{
    if (!c || n < 1 || n > 2) return fail(HVQ_E_ARG, "launch queues: 1 or 2");
    c->max_queues = n;
    return HVQ_OK;
}

/* The reuse window (hvq_launch_group_plan) the launches of one group of streams may span, in bytes; 0: a batch is never split.  Takes
 * effect at the next hvq_flush_begin. */
HVQ_EXPORT int hvq_context_set_group_bytes(HvqContext *c, uint64_t bytes)
{
    if (!c) return fail(HVQ_E_ARG, "null context");
    c->group_bytes = bytes;
    return HVQ_OK;
}

/* launch groups of the resident batch (the last one flushed), 0: none */
HVQ_EXPORT int hvq_context_launch_groups(HvqContext *c)
{
    if (!c) return fail(HVQ_E_ARG, "null context");
    { int rc = flush_end(c); if (rc) return rc; }
    return c->launches.empty() ? 0 : (int)c->groups;
}

HVQ_EXPORT void hvq_context_destroy(HvqContext *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)copy_join(c);
    (void)flush_end(c);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)export_drain(c);
    for (auto &s : c->streams) {
        if (s.parser) hvq_parser_destroy(s.parser);
        if (s.dev) (void)hipFree(s.dev);
        if (s.nest_keep) (void)hipFree(s.nest_keep);
    }
    for (auto &S : c->ps) {
        if (S.gp_dev) (void)hipFree(S.gp_dev);
        if (S.pj_dev) (void)hipFree(S.pj_dev);
        if (S.np_dev) (void)hipFree(S.np_dev);
        if (S.pr_host) (void)hipHostFree(S.pr_host);
        if (S.timing_dev) (void)hipFree(S.timing_dev);
        if (S.ev_parse) (void)hipEventDestroy(S.ev_parse);
        if (S.evp0) (void)hipEventDestroy(S.evp0);
        if (S.evp1) (void)hipEventDestroy(S.evp1);
    }
    if (c->host_arena) (void)hipHostFree(c->host_arena);
    if (c->redo_dev) (void)hipFree(c->redo_dev);
    if (c->rp_dev) (void)hipFree(c->rp_dev);
    if (c->dev_arena) (void)hipFree(c->dev_arena);
    if (c->host_arena_alt) (void)hipHostFree(c->host_arena_alt);
    if (c->dev_arena_alt) (void)hipFree(c->dev_arena_alt);
    for (auto &set : c->pin) for (auto &b : set) if (b.p) (void)hipHostFree(b.p);
    if (c->ev_copy) (void)hipEventDestroy(c->ev_copy);
    for (auto e : c->ev_arena_free) if (e) (void)hipEventDestroy(e);
    for (auto e : c->ev_h2d) if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->read_stream) { (void)hipStreamSynchronize(c->read_stream); (void)hipStreamDestroy(c->read_stream); }
    for (int q = 1; q < 4; ++q) {
        if (c->qstream[q]) { (void)hipStreamSynchronize(c->qstream[q]); (void)hipStreamDestroy(c->qstream[q]); }
        if (c->ev_join[q]) (void)hipEventDestroy(c->ev_join[q]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_read) (void)hipEventDestroy(c->ev_read);
    if (c->jobs_dev) (void)hipFree(c->jobs_dev);
    if (c->tq_dev) (void)hipFree(c->tq_dev);
    if (c->selfref_dev) (void)hipFree(c->selfref_dev);
    if (c->rb_dev) (void)hipFree(c->rb_dev);
    if (c->rb_tab_dev) (void)hipFree(c->rb_tab_dev);
    if (c->rb_tab_host) (void)hipHostFree(c->rb_tab_host);
    if (c->rgb_dev) (void)hipFree(c->rgb_dev);
    if (c->rgb_jobs_dev) (void)hipFree(c->rgb_jobs_dev);
    if (c->ck_acc) (void)hipFree(c->ck_acc);
    if (c->jp_scr) (void)hipFree(c->jp_scr);
    if (c->ph_acc) (void)hipFree(c->ph_acc);
    for (auto &t : c->ex) {
        if (t.host) (void)hipHostFree(t.host);
        if (t.dev) (void)hipFree(t.dev);
        if (t.ev) (void)hipEventDestroy(t.ev);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

/* bytes of a stream's picture ring ((nslots + 1) slots: the last one stays zero), 0 for a geometry the parser refuses.  Host only.
 * Every reference read of the kernels is ring base + 32-bit offset (HvqJob::ref0_off, block records, pair entries): the ring
 * must stay below 4 GiB, which hvq_stream_open enforces with this number. */
HVQ_EXPORT uint64_t hvq_stream_ring_bytes(int width, int height, int h_samp, int v_samp, int nslots)
{
    HvqParser *p = hvq_parser_create(width, height, h_samp, v_samp, 1);
    if (!p || nslots < 0) { if (p) hvq_parser_destroy(p); return 0; }
    const uint64_t slot = align_up((size_t)hvq_parser_pic_bytes(p) + 64, 256);
    hvq_parser_destroy(p);
    return ((uint64_t)nslots + 1u) * slot;
}

HVQ_EXPORT int hvq_stream_open(HvqContext *c, int width, int height, int h_samp, int v_samp, int is15, int nslots)
{
    if (!c) return fail(HVQ_E_ARG, "null context");
    if (nslots < 3) return fail(HVQ_E_ARG, "nslots must be >= 3 (past, present, future)");
    { int rcj = copy_join(c); if (rcj) return rcj; }
    HIPCHK(hipSetDevice(c->device));
    HvqParser *p = hvq_parser_create(width, height, h_samp, v_samp, is15);
    if (!p) return fail(HVQ_E_GEOMETRY, "unsupported geometry %dx%d sampling %dx%d (need multiples of 8, <= 8192; samplings 2x2, 1x1 and 2x1 -- the reference's own tables cannot decode 1x2)",
                        width, height, h_samp, v_samp);
    Stream s;
    s.open = true; s.parser = p; s.w = width; s.h = height;
    s.wshift = h_samp == 2; s.hshift = v_samp == 2;
    s.pic_bytes = hvq_parser_pic_bytes(p);
    s.slot_bytes = (uint32_t)align_up((size_t)s.pic_bytes + 64, 256);
    s.slots.resize((size_t)nslots);
    size_t bytes = (size_t)(nslots + 1) * s.slot_bytes;
    if (bytes >= ((size_t)1 << 32)) {
        hvq_parser_destroy(p);
        return fail(HVQ_E_OVERFLOW, "picture ring of %d + 1 slots x %u bytes exceeds 4 GiB (reference reads are ring base + 32-bit offset): open the stream with fewer slots",
                    nslots, s.slot_bytes);
    }
    hipError_t e = hipMalloc((void **)&s.dev, bytes);
    if (e != hipSuccess) { hvq_parser_destroy(p); return fail(HVQ_E_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    e = hipMemsetAsync(s.dev, 0, bytes, c->stream);
    if (e != hipSuccess) { hvq_parser_destroy(p); (void)hipFree(s.dev); return fail(HVQ_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e)); }
    c->streams.push_back(s);
    return (int)c->streams.size() - 1;
}

/* Host threads that share the parse of ONE picture of this stream (hvq_parser_set_threads: the picture's sections side by side; 1 = the
 * submitting thread alone, the default).  For callers that decode few streams (a lone clip: hvq_stream_submit parses its pictures one after
 * the other; hvq_submit_many parses streams side by side and leaves a stream's pictures to one thread).  Returns the count in effect. */
HVQ_EXPORT int hvq_stream_set_parse_threads(HvqContext *c, int sid, int threads)
{
    if (!c || sid < 0 || sid >= (int)c->streams.size() || !c->streams[sid].open) return fail(HVQ_E_ARG, "bad stream %d", sid);
    return hvq_parser_set_threads(c->streams[(size_t)sid].parser, threads);
}

HVQ_EXPORT int hvq_stream_close(HvqContext *c, int sid)
{
    if (!c || sid < 0 || sid >= (int)c->streams.size() || !c->streams[sid].open) return fail(HVQ_E_ARG, "bad stream %d", sid);
    for (auto &p : c->pending)
        if (p.stream == sid) return fail(HVQ_E_STATE, "stream %d has queued pictures; flush first", sid);
    { int rcj = copy_join(c); if (rcj) return rcj; }
    { int rc = flush_end(c); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(c->stream));
    { int rc = export_drain(c); if (rc) return rc; }
    Stream &s = c->streams[sid];
    hvq_parser_destroy(s.parser); s.parser = nullptr;
    HIPCHK(hipFree(s.dev)); s.dev = nullptr;
    if (s.nest_keep) { HIPCHK(hipFree(s.nest_keep)); s.nest_keep = nullptr; }
    c->launches.clear();               /* the resident batch may reference the freed slots: no replay after a close */
    s.open = false;
    return HVQ_OK;
}

HVQ_EXPORT uint32_t hvq_stream_pic_bytes(HvqContext *c, int sid)
{
    if (!c || sid < 0 || sid >= (int)c->streams.size() || !c->streams[sid].open) return 0;
    return c->streams[sid].pic_bytes;
}

static int alloc_slot(Stream &s)
{
    int n = (int)s.slots.size();
    for (int i = 0; i < n; ++i) {
        int cand = (s.ring + i) % n;
        if (cand != s.anchor_old && cand != s.anchor_new) { s.ring = (cand + 1) % n; return cand; }
    }
    return -1;
}

/* queue one picture: slot assignment == picture rotation of h4m:2087-2093 / 2131-2137, then the dependency level */
static int enqueue_common(HvqContext *c, int sid, int frame_type, Pending q)
{
    Stream &s = c->streams[(size_t)sid];
    q.stream = sid; q.ordinal = s.npics;
    if (frame_type != HVQ_FRAME_B) { std::swap(s.anchor_old, s.anchor_new); std::swap(s.rp_past, s.rp_future); }   /* past <-> future */
    /* where what the reference's `present` buffer holds right now lives here (looked up before the ring hands out a slot) */
    const int old_ord = s.rp_present;
    q.old_slot = old_ord < 0 ? -1 : (s.pic_slot[(size_t)old_ord] >= 0 ? s.pic_slot[(size_t)old_ord] : -2);
    q.host_old = s.sdk_present;
    s.rp_present = q.ordinal;
    if (frame_type != HVQ_FRAME_B) std::swap(s.rp_present, s.rp_future);
    q.dst = alloc_slot(s);
    if (frame_type == HVQ_FRAME_I) { q.ref0 = -1; q.ref1 = -1; }
    else if (frame_type == HVQ_FRAME_P) { q.ref0 = s.anchor_old; q.ref1 = q.dst; }  /* future aliases present, h4m:2060 */
    else { q.ref0 = s.anchor_old; q.ref1 = s.anchor_new; }
    int lvl = 0;
    auto dep_w = [&](int slot) { if (slot >= 0 && slot != q.dst) lvl = std::max(lvl, s.slots[slot].w_level + 1); };
    dep_w(q.ref0); dep_w(q.ref1);
    lvl = std::max(lvl, std::max(s.slots[q.dst].w_level, s.slots[q.dst].r_level) + 1);
    if (frame_type == HVQ_FRAME_P && q.old_slot >= 0 && q.old_slot != q.dst) {
        /* should the picture turn out to reference itself (known after its parse), that slot is read behind this level's launch:
         * complete by then, and not handed to a later picture before */
        lvl = std::max(lvl, s.slots[(size_t)q.old_slot].w_level);
        s.slots[(size_t)q.old_slot].r_level = std::max(s.slots[(size_t)q.old_slot].r_level, lvl);
    }
    q.level = lvl;
    if (q.ref0 >= 0) s.slots[q.ref0].r_level = std::max(s.slots[q.ref0].r_level, lvl);
    if (q.ref1 >= 0 && q.ref1 != q.dst) s.slots[q.ref1].r_level = std::max(s.slots[q.ref1].r_level, lvl);
    if (s.slots[q.dst].pic >= 0) s.pic_slot[(size_t)s.slots[q.dst].pic] = -1;
    s.slots[q.dst].w_level = lvl; s.slots[q.dst].r_level = -1; s.slots[q.dst].pic = q.ordinal;
    s.pic_slot.push_back(q.dst);
    if (frame_type != HVQ_FRAME_B) s.anchor_new = q.dst;     /* present <-> future: newest anchor becomes "future" */
    c->pending.push_back(q);
    return s.npics++;
}

/* host-parsed picture: blob already in the host arena at `off` */
static int enqueue_picture(HvqContext *c, int sid, int frame_type, size_t off, size_t blen)
{
    Pending q{};
    q.blob_off = off; q.blob_len = blen;
    const HvqPicHeader *hd = (const HvqPicHeader *)(c->host_arena + off);
    q.ntiles = hd->tile_first[3]; q.nwg = picture_workgroups(hd->tile_first);
    q.kind = hd->pic_kind; q.w = hd->width; q.h = hd->height;
    q.max_items = hd->max_items; q.max_pairs = hd->max_pairs;
    return enqueue_common(c, sid, frame_type, q);
}

static int check_submit_args(HvqContext *c, int sid, int frame_type, const uint8_t *pic, size_t len, bool check_resume = true)
{
    if (!c || sid < 0 || sid >= (int)c->streams.size() || !c->streams[sid].open) return fail(HVQ_E_ARG, "bad stream %d", sid);
    if (!pic || len < 8 + 0x44 + 4) return fail(HVQ_E_ARG, "picture too short (%zu bytes)", len);
    if (frame_type != HVQ_FRAME_I && frame_type != HVQ_FRAME_P && frame_type != HVQ_FRAME_B)
        return fail(HVQ_E_ARG, "unknown frame type 0x%x", frame_type);
    if (check_resume && c->streams[sid].need_I && frame_type != HVQ_FRAME_I)
        return fail(HVQ_E_STATE, "stream %d: a picture was rejected, decoding resumes at the next I picture", sid);
    return HVQ_OK;
}

/* the same rule over a list of pictures: an I picture earlier in the list re-opens its stream for the ones after it */
static int check_resume_order(HvqContext *c, int n, const int *streams, const int *frame_types)
{
    std::vector<char> need(c->streams.size());
    for (size_t i = 0; i < need.size(); ++i) need[i] = c->streams[i].need_I;
    for (int i = 0; i < n; ++i) {
        if (frame_types[i] == HVQ_FRAME_I) need[(size_t)streams[i]] = 0;
        else if (need[(size_t)streams[i]])
            return fail(HVQ_E_STATE, "stream %d: a picture was rejected, decoding resumes at the next I picture", streams[i]);
    }
    return HVQ_OK;
}

HVQ_EXPORT int hvq_stream_submit(HvqContext *c, int sid, int frame_type, const uint8_t *pic, size_t len)
{
    int rc = check_submit_args(c, sid, frame_type, pic, len);
    if (rc) return rc;
    rc = copy_join(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    Stream &s = c->streams[sid];
    if (s.parse_mode == 2) return fail(HVQ_E_STATE, "stream %d is parsed on the GPU; use hvq_submit_many_device", sid);
    s.parse_mode = 1;
    size_t bound = align_up(hvq_parser_blob_bound(s.parser), 256);
    rc = arena_reserve(c, bound);
    if (rc) return rc;
    size_t off = c->arena_used, blen = 0;
    auto t0 = std::chrono::steady_clock::now();
    rc = hvq_parse_picture(s.parser, frame_type, pic, len, c->host_arena + off, bound, &blen);
    c->parse_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc) return fail(rc, "parse failed (%d) for stream %d picture %d", rc, sid, s.npics);
    /* the header's flags plus what a P/B picture's second pass raised behind it (an endless overflow run in a block's scalars, a
     * clamped vector target): refused, never decoded differently */
    if (const char *why = unsupported_reason(((const HvqPicHeader *)(c->host_arena + off))->flags | hvq_parser_last_flags(s.parser))) {
        s.need_I = true;
        return fail(HVQ_E_UNSUPPORTED, "stream %d picture %d: %s", sid, s.npics, why);
    }
    if (frame_type == HVQ_FRAME_I) s.need_I = false;
    c->arena_used = off + align_up(blen, 256);
    return enqueue_picture(c, sid, frame_type, off, blen);
}

HVQ_EXPORT int hvq_submit_many(HvqContext *c, int n, const int *streams, const int *frame_types,
                               const uint8_t *const *pics, const size_t *lens, int threads, int *ordinals)
{
    if (!c || n < 0 || !streams || !frame_types || !pics || !lens) return fail(HVQ_E_ARG, "bad arguments");
    for (int i = 0; i < n; ++i) {
        int rc = check_submit_args(c, streams[i], frame_types[i], pics[i], lens[i], false);
        if (rc) return rc;
    }
    if (n == 0) return HVQ_OK;
    { int rcj = copy_join(c); if (rcj) return rcj; }
    { int rc = check_resume_order(c, n, streams, frame_types); if (rc) return rc; }
    for (int i = 0; i < n; ++i) {
        Stream &s = c->streams[(size_t)streams[i]];
        if (s.parse_mode == 2) return fail(HVQ_E_STATE, "stream %d is parsed on the GPU; use hvq_submit_many_device", streams[i]);
        s.parse_mode = 1;
    }
    HIPCHK(hipSetDevice(c->device));
    threads = std::max(1, std::min(threads, 256));
    /* work units = streams (a parser is stateful); unit u gets its pictures in array order */
    std::vector<std::vector<int>> per_stream(c->streams.size());
    std::vector<int> units;
    for (int i = 0; i < n; ++i) {
        if (per_stream[(size_t)streams[i]].empty()) units.push_back(streams[i]);
        per_stream[(size_t)streams[i]].push_back(i);
    }
    /* workers parse into private growing buffers (no per-picture allocation), then copy their blobs into the
     * pinned arena in parallel once the layout is known */
    struct Piece { int worker; size_t off, len; uint32_t late; };     /* late: flags raised behind the blob header (hvq_parser_last_flags) */
    std::vector<Piece> pieces((size_t)n, Piece{ -1, 0, 0, 0 });
    std::vector<int> rcs((size_t)n, 0);
    struct RawBuf {                       /* growing byte buffer without value-initialisation */
        uint8_t *p = nullptr; size_t size = 0, cap = 0;
        ~RawBuf() { free(p); }
        bool ensure(size_t n) { if (n <= cap) return true; size_t nc = std::max(cap * 2, n); uint8_t *q = (uint8_t *)realloc(p, nc); if (!q) return false; p = q; cap = nc; return true; }
    };
    std::vector<RawBuf> wbuf((size_t)threads);
    std::atomic<size_t> next{ 0 };
    auto t0 = std::chrono::steady_clock::now();
    auto worker = [&](int wid) {
        RawBuf &buf = wbuf[(size_t)wid];
        for (;;) {
            size_t u = next.fetch_add(1);
            if (u >= units.size()) break;
            Stream &s = c->streams[(size_t)units[u]];
            const size_t bound = hvq_parser_blob_bound(s.parser);
            for (int i : per_stream[(size_t)units[u]]) {
                if (!buf.ensure(buf.size + bound + 32)) { rcs[(size_t)i] = HVQ_E_OVERFLOW; break; }
                const size_t at = (size_t)((((uintptr_t)buf.p + buf.size + 15) & ~(uintptr_t)15) - (uintptr_t)buf.p);
                size_t blen = 0;
                rcs[(size_t)i] = hvq_parse_picture(s.parser, frame_types[i], pics[i], lens[i], buf.p + at, bound, &blen);
                if (rcs[(size_t)i]) break;                 /* later pictures of the stream would see a wrong parser state */
                pieces[(size_t)i] = Piece{ wid, at, blen, hvq_parser_last_flags(s.parser) };
                buf.size = at + blen;
            }
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) pool.emplace_back(worker, t);
        worker(0);
        for (auto &t : pool) t.join();
    }
    for (int i = 0; i < n; ++i)
        if (rcs[(size_t)i] || pieces[(size_t)i].worker < 0)
            return fail(rcs[(size_t)i] ? rcs[(size_t)i] : HVQ_E_STATE, "parse failed for picture %d (stream %d)", i, streams[i]);
    for (int i = 0; i < n; ++i) {
        const Piece &pc = pieces[(size_t)i];
        if (const char *why = unsupported_reason(((const HvqPicHeader *)(wbuf[(size_t)pc.worker].p + pc.off))->flags | pc.late)) {
            c->streams[(size_t)streams[i]].need_I = true;
            return fail(HVQ_E_UNSUPPORTED, "picture %d (stream %d): %s; nothing of this call was queued", i, streams[i], why);
        }
    }
    for (int i = 0; i < n; ++i) if (frame_types[i] == HVQ_FRAME_I) c->streams[(size_t)streams[i]].need_I = false;
    size_t need = 0;
    std::vector<size_t> offs((size_t)n);
    for (int i = 0; i < n; ++i) { offs[(size_t)i] = need; need += align_up(pieces[(size_t)i].len, 256); }
    int rc = arena_reserve(c, need);
    if (rc) return rc;
    const size_t base = c->arena_used;
    {
        std::atomic<int> nexti{ 0 };
        auto copier = [&]() {
            for (;;) {
                int i = nexti.fetch_add(1);
                if (i >= n) break;
                const Piece &pc = pieces[(size_t)i];
                memcpy(c->host_arena + base + offs[(size_t)i], wbuf[(size_t)pc.worker].p + pc.off, pc.len);
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) pool.emplace_back(copier);
        copier();
        for (auto &t : pool) t.join();
    }
    c->parse_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < n; ++i) {
        int ord = enqueue_picture(c, streams[i], frame_types[i], base + offs[(size_t)i], pieces[(size_t)i].len);
        if (ordinals) ordinals[i] = ord;
    }
    c->arena_used = base + need;
    return HVQ_OK;
}

/* GPU entropy parse: queue the raw bitstreams; hvq_flush parses them on the device (hvq_gparse.hip).  Three ways for the bytes to
 * reach the pinned arena:
 *   SUBMIT_COPY        copied before the call returns (hvq_submit_many_device: the caller's buffers are free again on return)
 *   SUBMIT_COPY_ASYNC  copied by a worker thread (hvq_submit_many_device_async: the buffers stay the caller's until the next
 *                      hvq_flush_begin / hvq_sync joins the worker)
 *   SUBMIT_ARENA       already there: the caller filled a reservation of the arena itself (hvq_arena_reserve) -- no copy at all */
enum SubmitMode { SUBMIT_COPY, SUBMIT_COPY_ASYNC, SUBMIT_ARENA };
static int submit_device(HvqContext *c, int n, const int *streams, const int *frame_types, const uint8_t *const *pics_in,
                         const size_t *arena_offs, const size_t *lens, int *ordinals, SubmitMode mode)
{
    if (!c || n < 0 || !streams || !frame_types || !lens || (mode == SUBMIT_ARENA ? !arena_offs : !pics_in)) return fail(HVQ_E_ARG, "bad arguments");
    size_t need = 0;
    { int rcj = copy_join(c); if (rcj) return rcj; }
    std::vector<const uint8_t *> arena_pics;
    if (mode == SUBMIT_ARENA) {
        if (!c->resv_active) return fail(HVQ_E_STATE, "no arena reservation outstanding (hvq_arena_reserve)");
        arena_pics.resize((size_t)n);
        size_t prev_end = 0;
        for (int i = 0; i < n; ++i) {
            if (lens[i] > c->resv_bytes)               /* before the span is computed: lens[i] + 32 must not wrap */
                return fail(HVQ_E_ARG, "picture %d: %zu bytes exceed the reservation (%zu)", i, lens[i], c->resv_bytes);
            const size_t span = align_up(lens[i] + 32, 256);
            if ((arena_offs[i] & 255u) || arena_offs[i] < prev_end || arena_offs[i] > c->resv_bytes || span > c->resv_bytes - arena_offs[i])
                return fail(HVQ_E_ARG, "picture %d: offset %zu (+ %zu bytes with its padding) is not a 256-byte aligned, ascending range of the reservation", i, arena_offs[i], span);
            prev_end = arena_offs[i] + span;
            arena_pics[(size_t)i] = c->host_arena + c->resv_base + arena_offs[i];
        }
    }
    const uint8_t *const *pics = mode == SUBMIT_ARENA ? arena_pics.data() : pics_in;
    for (int i = 0; i < n; ++i) {
        int rc = check_submit_args(c, streams[i], frame_types[i], pics[i], lens[i], false);
        if (rc) return rc;
        if (lens[i] > 0x7FFFFFF0u) return fail(HVQ_E_ARG, "picture %d: the GPU parser needs the real picture length", i);
        if (c->streams[(size_t)streams[i]].parse_mode == 1)
            return fail(HVQ_E_STATE, "stream %d is parsed on the host; a stream keeps one parser for its lifetime", streams[i]);
        need += align_up(lens[i] + 32, 256);
    }
    if (n == 0) { if (mode == SUBMIT_ARENA) c->resv_active = false; return HVQ_OK; }
    { int rcr = check_resume_order(c, n, streams, frame_types); if (rcr) return rcr; }
    HIPCHK(hipSetDevice(c->device));
    if (mode != SUBMIT_ARENA) {
        int rc = arena_reserve(c, need);
        if (rc) return rc;
    }
    std::vector<size_t> offs((size_t)n);
    /* Everything below changes stream and queue state before the last thing that can fail (allocation, upload): a failed
     * call must leave the context as it found it, so the touched streams are saved and put back. */
    std::vector<std::pair<int, Stream>> saved;
    const size_t pend0 = c->pending.size(), used0 = c->arena_used;
    auto rollback = [&]() {
        for (auto &kv : saved) {
            Stream &s = c->streams[(size_t)kv.first];
            if (s.nest_keep && !kv.second.nest_keep) (void)hipFree(s.nest_keep);
            s = kv.second;
        }
        c->pending.resize(pend0);
        c->arena_used = used0;
        if (c->arena_uploaded > used0) c->arena_uploaded = used0;
    };
#define HIPCHK_RB(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { rollback(); return fail(HVQ_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); } } while (0)
    for (int i = 0; i < n; ++i) {
        Stream &s = c->streams[(size_t)streams[i]];
        {
            bool have = false;
            for (auto &kv : saved) have |= kv.first == streams[i];
            if (!have) saved.emplace_back(streams[i], s);
        }
        if (s.parse_mode == 0) {
            s.parse_mode = 2;
            hvq_parser_layout(s.parser, &s.layout);
            s.blob_cap = (uint32_t)align_up(hvq_parser_blob_bound(s.parser), 256);
            uint32_t blocks = 0;
            for (int k = 0; k < 3; ++k) blocks += (uint32_t)s.layout.hb[k] * s.layout.vb[k];
            s.scratch_bytes = (uint32_t)align_up(hvq_gparse_scratch_bytes(blocks, s.layout.tile_first[3] * (HVQ_TILE_BLOCKS / 64),
                                                                          s.layout.mcb_w * s.layout.mcb_h), 256);
            HIPCHK_RB(hipMalloc((void **)&s.nest_keep, 2 * GP_ALIGN16(HVQ_NESTP_BYTES)));
            HIPCHK_RB(hipMemsetAsync(s.nest_keep, 0, 2 * GP_ALIGN16(HVQ_NESTP_BYTES), c->stream));
        }
        if (mode == SUBMIT_ARENA) offs[(size_t)i] = c->resv_base + arena_offs[i];      /* arena_used already covers the reservation */
        else { offs[(size_t)i] = c->arena_used; c->arena_used += align_up(lens[i] + 32, 256); }
        Pending q{};
        q.dev = true;
        q.blob_off = offs[(size_t)i]; q.blob_len = lens[i];
        q.ntiles = s.layout.tile_first[3]; q.nwg = picture_workgroups(s.layout.tile_first);
        q.kind = frame_types[i] == HVQ_FRAME_I ? HVQ_PIC_I : (frame_types[i] == HVQ_FRAME_P ? HVQ_PIC_P : HVQ_PIC_B);
        q.w = s.layout.width; q.h = s.layout.height;
        q.unk_shift = pics[i][1];
        q.nest_ref = s.nest_src;
        const int ord = enqueue_common(c, streams[i], frame_types[i], q);
        if (frame_types[i] == HVQ_FRAME_I) {
            s.need_I = false;
            s.nest_src = (int)c->pending.size() - 1;
            c->pending.back().nest_ref = s.nest_src;
        }
        if (ordinals) ordinals[i] = ord;
    }
    /* bitstreams -> pinned arena -> HBM, pipelined: a few threads copy a chunk of pictures (zero padded: the device
     * reader sees zeros past the end), its H2D is queued at once and runs while the next chunk is being copied.
     * While a batch is in flight (streaming: hvq_flush_begin ... hvq_flush_end) the copy runs on a worker thread and this call
     * returns at once, so that the caller reaches hvq_flush_end -- and the in-flight batch its reconstruction launches -- as soon as
     * the parse results arrive, however long the host takes over 160 MB of memcpy (4-7.5 ms on a shared host, measured); the next
     * hvq_flush_begin joins the worker.  `pics[i]` must stay readable until then. */
    struct CopyJob { std::vector<const uint8_t *> pics; std::vector<size_t> lens, offs; size_t end_used; bool early; uint8_t *host; };
    CopyJob job;
    job.pics.assign(pics, pics + n); job.lens.assign(lens, lens + n); job.offs = offs;
    job.end_used = c->arena_used; job.early = c->arena_uploaded == offs[0];          /* nothing older is waiting for the flush-time upload */
    job.host = c->host_arena;
    auto run_copy = [c](const CopyJob &j) -> int {
        const int n = (int)j.pics.size();
        const auto tc0 = std::chrono::steady_clock::now();
        /* chunks of ~16 MB: a chunk's H2D is queued as soon as its last picture is in the arena.  The copy threads are started ONCE
         * per batch and take pictures off a shared counter (round 3 started and joined a set of threads per chunk: 70 thread
         * starts per 160 MB batch); the calling thread copies too and queues the uploads in chunk order. */
        const size_t chunk_bytes = (size_t)16 << 20;
        std::vector<int> chunk_end;                         /* picture index behind each chunk */
        {
            size_t bytes = 0;
            for (int i = 0; i < n; ++i) {
                bytes += align_up(j.lens[(size_t)i] + 32, 256);
                if (bytes >= chunk_bytes || i == n - 1) { chunk_end.push_back(i + 1); bytes = 0; }
            }
        }
        std::vector<std::atomic<int>> left(chunk_end.size());
        for (size_t k = 0; k < chunk_end.size(); ++k) left[k].store(chunk_end[k] - (k ? chunk_end[k - 1] : 0));
        std::vector<int> chunk_of((size_t)n);
        for (size_t k = 0, i = 0; k < chunk_end.size(); ++k) for (; (int)i < chunk_end[k]; ++i) chunk_of[i] = (int)k;
        std::atomic<int> next{ 0 };
        auto copy_some = [&](int budget) {               /* up to `budget` pictures; returns false when none was left */
            bool any = false;
            while (budget-- > 0) {
                const int i = next.fetch_add(1);
                if (i >= n) return any;
                uint8_t *dst = j.host + j.offs[(size_t)i];
                const size_t span = align_up(j.lens[(size_t)i] + 32, 256);
                copy_to_arena(dst, j.pics[(size_t)i], j.lens[(size_t)i]);
                memset(dst + j.lens[(size_t)i], 0, span - j.lens[(size_t)i]);
#if defined(__x86_64__)
                _mm_sfence();                            /* the streamed lines are in memory before the chunk's upload is queued */
#else
                std::atomic_thread_fence(std::memory_order_seq_cst);
#endif
                left[(size_t)chunk_of[(size_t)i]].fetch_sub(1, std::memory_order_release);
                any = true;
            }
            return true;
        };
        size_t total = 0;
        for (int i = 0; i < n; ++i) total += j.lens[(size_t)i];
        /* 8 threads when the host has them: with 4 the copy of a dense batch (160 MB) takes about as long as the GPU leaves for it */
        static const int copy_threads = getenv("HVQM4_AMD_COPY_THREADS") ? std::max(1, atoi(getenv("HVQM4_AMD_COPY_THREADS")))
                                                                         : (std::thread::hardware_concurrency() >= 16 ? 8 : 4);
        const int nt = total >= ((size_t)4 << 20) ? copy_threads : 1;
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; ++t) pool.emplace_back([&]() { while (copy_some(1 << 30)) {} });
        int rc = HVQ_OK;
        for (size_t k = 0; k < chunk_end.size(); ++k) {
            while (left[k].load(std::memory_order_acquire) > 0)
                if (!copy_some(4)) std::this_thread::yield();      /* help; when nothing is left to take, wait for the others */
            if (j.early && !rc) rc = arena_upload(c, k + 1 < chunk_end.size() ? j.offs[(size_t)chunk_end[k]] : j.end_used);
        }
        for (auto &t : pool) t.join();
        c->copy_bytes += total;
        c->copy_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tc0).count();
        /* test hook (tests/test_gpu_batch.py): the upload of this batch "fails" -- exercises the rollback of both copy modes */
        if (!rc && getenv("HVQM4_AMD_TEST_FAIL_COPY")) rc = fail(HVQ_E_HIP, "bitstream upload failed (HVQM4_AMD_TEST_FAIL_COPY)");
        return rc;
    };
    if (mode == SUBMIT_ARENA) {
        /* the bytes are in place: zero the padding behind every picture (the device reader sees zeros past the end) and queue the
         * upload of the whole reservation at once */
        for (int i = 0; i < n; ++i) {
            uint8_t *dst = c->host_arena + offs[(size_t)i];
            memset(dst + lens[i], 0, align_up(lens[i] + 32, 256) - lens[i]);
        }
        c->resv_active = false;
        if (c->arena_uploaded == c->resv_base) {                    /* nothing older is waiting for the flush-time upload */
            int rcu = arena_upload(c, c->resv_base + c->resv_bytes);
            if (rcu) { rollback(); return rcu; }
        }
        return HVQ_OK;
    }
    /* only the _async entry point defers its copy (rounds 4-5 had an environment switch that made the plain call defer too: a caller
     * of the plain call may free its buffers on return, so the switch was a use-after-free waiting to happen; removed in round 6) */
    if (mode == SUBMIT_COPY_ASYNC) {
        c->copy_rc = HVQ_OK;
        c->copy_err.clear();
        c->copy_active = true;
        c->copy_done.store(false, std::memory_order_relaxed);
        const int dev = c->device;
        c->copy_worker = std::thread([c, dev, run_copy, job = std::move(job)]() {
            (void)hipSetDevice(dev);
            c->copy_rc = run_copy(job);
            if (c->copy_rc) c->copy_err = g_err;          /* the worker's thread-local error text */
            c->copy_done.store(true, std::memory_order_release);
        });
    } else {
        int rcc = run_copy(job);
        if (rcc) { rollback(); return rcc; }
    }
#undef HIPCHK_RB
    return HVQ_OK;
}

HVQ_EXPORT int hvq_submit_many_device(HvqContext *c, int n, const int *streams, const int *frame_types,
                                      const uint8_t *const *pics, const size_t *lens, int *ordinals)
{
    return submit_device(c, n, streams, frame_types, pics, nullptr, lens, ordinals, SUBMIT_COPY);
}

HVQ_EXPORT int hvq_submit_many_device_async(HvqContext *c, int n, const int *streams, const int *frame_types,
                                            const uint8_t *const *pics, const size_t *lens, int *ordinals)
{
    return submit_device(c, n, streams, frame_types, pics, nullptr, lens, ordinals, SUBMIT_COPY_ASYNC);
}

/* Zero-copy submit: the caller fills a reservation of the pinned arena itself (a container reader read()s file bytes straight into
 * it), so the 160 MB per batch the copying calls move through the host's caches and DRAM once more never move at all. */
HVQ_EXPORT int hvq_arena_reserve(HvqContext *c, size_t bytes, void **ptr)
{
    if (!c || !ptr || bytes == 0) return fail(HVQ_E_ARG, "bad arguments");
    { int rcj = copy_join(c); if (rcj) return rcj; }
    if (c->resv_active) return fail(HVQ_E_STATE, "an arena reservation is outstanding already: submit it (hvq_submit_many_arena) first");
    HIPCHK(hipSetDevice(c->device));
    const size_t base = align_up(c->arena_used, 256);
    bytes = align_up(bytes, 256);
    { int rc = arena_reserve(c, base - c->arena_used + bytes); if (rc) return rc; }
    if (c->arena_uploaded == c->arena_used) c->arena_uploaded = base;      /* the alignment gap carries nothing */
    c->resv_base = base; c->resv_bytes = bytes; c->resv_active = true;
    c->arena_used = base + bytes;
    *ptr = c->host_arena + base;
    return HVQ_OK;
}

HVQ_EXPORT size_t hvq_arena_stride(size_t len) { return align_up(len + 32, 256); }

HVQ_EXPORT int hvq_submit_many_arena(HvqContext *c, int n, const int *streams, const int *frame_types,
                                     const size_t *offsets, const size_t *lens, int *ordinals)
{
    return submit_device(c, n, streams, frame_types, nullptr, offsets, lens, ordinals, SUBMIT_ARENA);
}

/* GPU-parsed pictures of the pending batch: lay their blobs out, queue the parse kernel and the read-back of its
 * results on the compute stream (which already waits for the bitstreams' H2D).  Nothing here waits for the GPU. */
static int device_parse_launch(HvqContext *c)
{
    std::vector<size_t> &idx = PS(c).fl_idx;
    idx.clear();
    size_t need = 0;
    uint32_t rowbuf = 0;
    for (size_t i = 0; i < c->pending.size(); ++i) {
        Pending &p = c->pending[i];
        if (!p.dev) continue;
        const Stream &s = c->streams[(size_t)p.stream];
        idx.push_back(i);
        need += (size_t)s.blob_cap + s.scratch_bytes + align_up(GP_ALIGN16(HVQ_NESTP_BYTES), 256);
        rowbuf = std::max(rowbuf, (uint32_t)s.layout.hb[0] + 2u);
    }
    if (idx.empty()) return HVQ_OK;
    if (need > PS(c).gp_cap) {
        if (PS(c).gp_dev) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(PS(c).gp_dev)); PS(c).gp_dev = nullptr; PS(c).gp_cap = 0; }
        HIPCHK(hipMalloc((void **)&PS(c).gp_dev, need));
        PS(c).gp_cap = need;
    }
    if (idx.size() > PS(c).pj_cap) {
        if (PS(c).pj_dev) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(PS(c).pj_dev)); HIPCHK(hipFree(PS(c).np_dev)); }
        PS(c).pj_cap = idx.size() * 2;
        HIPCHK(hipMalloc((void **)&PS(c).pj_dev, PS(c).pj_cap * sizeof(HvqParseJob)));
        HIPCHK(hipMalloc((void **)&PS(c).np_dev, PS(c).pj_cap * 2 * sizeof(uint64_t)));
    }
    if (idx.size() > PS(c).pr_host_cap) {
        if (PS(c).pr_host) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipHostFree(PS(c).pr_host)); }
        PS(c).pr_host_cap = idx.size() * 2;
        HIPCHK(hipHostMalloc((void **)&PS(c).pr_host, PS(c).pr_host_cap * sizeof(HvqParseResult), hipHostMallocDefault));
    }
    std::vector<HvqParseJob> &jobs = PS(c).pjobs_host;
    jobs.assign(idx.size(), HvqParseJob{});
    size_t off = 0;
    for (size_t k = 0; k < idx.size(); ++k) {
        Pending &p = c->pending[idx[k]];
        const Stream &s = c->streams[(size_t)p.stream];
        HvqParseJob &j = jobs[k];
        p.dev_blob = (uint64_t)(uintptr_t)(PS(c).gp_dev + off);             off += s.blob_cap;
        j.scratch = (uint64_t)(uintptr_t)(PS(c).gp_dev + off);              off += s.scratch_bytes;
        p.dev_nest = (uint64_t)(uintptr_t)(PS(c).gp_dev + off);             off += align_up(GP_ALIGN16(HVQ_NESTP_BYTES), 256);
        j.pic = (uint64_t)(uintptr_t)(c->dev_arena + p.blob_off);
        j.blob = p.dev_blob;
        j.nest_out = p.dev_nest;
        j.len = (uint32_t)p.blob_len;
        j.pic_dwords = (uint32_t)((p.blob_len + 32) / 4);     /* zero padding the flat parse path may look into (gf_setup_lanes) */
        j.cap = s.blob_cap;
        j.width = (uint16_t)p.w; j.height = (uint16_t)p.h;
        j.frame_type = (uint8_t)(p.kind == HVQ_PIC_I ? HVQ_FRAME_I : (p.kind == HVQ_PIC_P ? HVQ_FRAME_P : HVQ_FRAME_B));
        j.h_samp = s.layout.wshift ? 2 : 1; j.v_samp = s.layout.hshift ? 2 : 1;
        j.is15 = (s.layout.flags & HVQ_F_IS15) ? 1 : 0;
    }
    { int rcu = staged_upload(c, c->arena_id, 0, PS(c).pj_dev, jobs.data(), jobs.size() * sizeof(HvqParseJob)); if (rcu) return rcu; }
    HIPCHK(hipEventRecord(PS(c).evp0, c->stream));
    /* HVQM4_AMD_PARSE_TIMING=1: per-phase times of the parse kernel (development aid, prints to stderr) */
    static const bool want_timing = getenv("HVQM4_AMD_PARSE_TIMING") != nullptr;
    PS(c).timing_dev = nullptr;
    if (want_timing) {
        HIPCHK(hipMalloc((void **)&PS(c).timing_dev, jobs.size() * 16 * sizeof(uint64_t)));
        HIPCHK(hipMemsetAsync(PS(c).timing_dev, 0, jobs.size() * 16 * sizeof(uint64_t), c->stream));
    }
    /* HVQM4_AMD_PARSE_FLAT=0: round 1's chains only (the flat path falls back to them by itself where it has to) */
    static const bool use_flat = !(getenv("HVQM4_AMD_PARSE_FLAT") && atoi(getenv("HVQM4_AMD_PARSE_FLAT")) == 0);
    PS(c).fl_rowbuf = rowbuf;
    /* The parse workgroups write their result records straight into pinned host memory (one 48-byte record per picture).  A
     * read-back copy queued behind the parse kernel would sit on a DMA engine for the whole parse -- and every second batch the
     * NEXT batch's bitstream uploads (copy stream) were dealt to that same engine and started only when the parse ended: periods
     * of 6.2 and 8.4 ms alternating (kernel and copy trace, profiles/r04g_streaming_timeline.txt). */
#ifdef GP_PROBE
    /* probe build: HVQM4_AMD_PARSE_EXIT=<stamp> runs the flat kernel up to that stamp first (its own events, time on stderr) */
    if (const char *ex = getenv("HVQM4_AMD_PARSE_EXIT")) {
        static hipEvent_t pe0 = nullptr, pe1 = nullptr;
        static float last_ms = -1.f;
        if (!pe0) { HIPCHK(hipEventCreate(&pe0)); HIPCHK(hipEventCreate(&pe1)); }
        else if (hipEventQuery(pe1) == hipSuccess) { float pm = 0; if (hipEventElapsedTime(&pm, pe0, pe1) == hipSuccess) last_ms = pm; }
        if (last_ms >= 0) fprintf(stderr, "hvqm4_amd parse probe: exit at stamp %d: %.3f ms (previous batch)\n", atoi(ex), last_ms);
        HIPCHK(hipEventRecord(pe0, c->stream));
        HIPCHK(hvq_launch_parse_probe(PS(c).pj_dev, PS(c).pr_host, (uint32_t)jobs.size(), rowbuf, (uint32_t)atoi(ex), c->stream));
        HIPCHK(hipEventRecord(pe1, c->stream));
        HIPCHK(hipEventRecord(PS(c).evp0, c->stream));
    }
#endif
    HIPCHK(hvq_launch_parse(PS(c).pj_dev, PS(c).pr_host, (uint32_t)jobs.size(), rowbuf, use_flat ? 1u : 0u, nullptr, PS(c).timing_dev, c->stream));
    HIPCHK(hipEventRecord(PS(c).evp1, c->stream));
    HIPCHK(hipEventRecord(PS(c).ev_parse, c->stream));
    return HVQ_OK;
}

static size_t jobs_len_of(const HvqContext *c, size_t k) { return k < PS(c).pjobs_host.size() ? (size_t)PS(c).pjobs_host[k].len : 0; }

/* wait for the parse results of the batch in flight and take them over */
static int device_parse_finish(HvqContext *c)
{
    const std::vector<size_t> &idx = PS(c).fl_idx;
    if (idx.empty()) return HVQ_OK;
    {   /* The reconstruction launches wait for this thread to have seen the parse results: the GPU idles for as long as the wake-up
         * takes.  Polling the event costs this thread a core for the length of the parse kernel and takes the results some tens of
         * microseconds earlier than the driver's wait (HVQM4_AMD_SPIN_WAIT=0: the driver's wait). */
        static const bool spin = !(getenv("HVQM4_AMD_SPIN_WAIT") && atoi(getenv("HVQM4_AMD_SPIN_WAIT")) == 0);
        if (spin) {
            hipError_t q;
            while ((q = hipEventQuery(PS(c).ev_parse)) == hipErrorNotReady) { for (int k = 0; k < 32; ++k) cpu_relax(); }
            HIPCHK(q);
        } else HIPCHK(hipEventSynchronize(PS(c).ev_parse));
    }
    const HvqParseResult *res = PS(c).pr_host;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, PS(c).evp0, PS(c).evp1));
    c->gpu_parse_ms = ms;
    /* Pictures the flat parse path could not serve (sections in an unusual order, array capacities, overflow groups at
     * the chains' caps) come back marked: the chains kernel parses those, same blobs as they would have been. */
    uint32_t n_redo = 0;
    {
        std::vector<uint32_t> redo;
        for (size_t k = 0; k < idx.size(); ++k) if (res[k].pad[0] == 2u) redo.push_back((uint32_t)k);
        n_redo = (uint32_t)redo.size();
        if (n_redo) {
            if (redo.size() > c->redo_cap) {
                if (c->redo_dev) { HIPCHK(hipFree(c->redo_dev)); c->redo_dev = nullptr; c->redo_cap = 0; }
                HIPCHK(hipMalloc((void **)&c->redo_dev, redo.size() * 2 * sizeof(uint32_t)));
                c->redo_cap = redo.size() * 2;
            }
            HIPCHK(hipMemcpyAsync(c->redo_dev, redo.data(), redo.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipEventRecord(c->ev0, c->stream));
            HIPCHK(hvq_launch_parse(PS(c).pj_dev, PS(c).pr_host, n_redo, PS(c).fl_rowbuf, 0u, c->redo_dev, nullptr, c->stream));
            HIPCHK(hipEventRecord(c->ev1, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));       /* also keeps `redo` alive until its upload is done */
            float ms2 = 0;
            HIPCHK(hipEventElapsedTime(&ms2, c->ev0, c->ev1));
            c->gpu_parse_ms += ms2;                        /* the parse time of the batch includes the second launch */
        }
    }
    const bool want_timing_print = PS(c).timing_dev != nullptr;
    if (PS(c).timing_dev) {
        std::vector<uint64_t> tm(idx.size() * 16);
        HIPCHK(hipMemcpy(tm.data(), PS(c).timing_dev, tm.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIPCHK(hipFree(PS(c).timing_dev)); PS(c).timing_dev = nullptr;
        /* stamp k of hvq_parse_kernel (GP_STAMP): average time since the picture's start, in the order they happened */
        static const char *label[16] = { "start", "trees", "mb types", "DC placed", "run sums", "chains ready or decoder", "coefficients/scans",
                                         "merge", "run scan", "entries", "emit count", "emit scan or MV x", "tags+lists", "kinds/DC or lanes",
                                         "expansions", "MV y" };
        double sum[3][16] = {}; size_t cnt[3][16] = {}, pics[3] = {}; uint64_t t_min = ~0ull, t_max = 0;
        uint64_t s_max = 0, d_min = ~0ull, d_max = 0, k_max[3] = { 0, 0, 0 }, k_end[3] = { 0, 0, 0 };
        if (getenv("HVQM4_AMD_PARSE_PROF"))
            for (size_t k = 0; k < idx.size() && k < 16; ++k)
                fprintf(stderr, "prof picture %zu kind %d: wait part %llu  decode part %llu  rounds %llu (shader clocks)\n", k, (int)c->fl_pending[idx[k]].kind,
                        (unsigned long long)tm[16 * k + 9], (unsigned long long)tm[16 * k + 10], (unsigned long long)tm[16 * k + 6]);
        for (size_t k = 0; k < idx.size(); ++k) {
            const uint64_t *t = &tm[16 * k];
            const int kind = (int)c->fl_pending[idx[k]].kind;
            for (int ph = 1; ph < 16; ++ph) if (t[ph]) { sum[kind][ph] += (double)(t[ph] - t[0]) * 0.01; cnt[kind][ph]++; }
            pics[kind]++; t_min = std::min(t_min, t[0]); t_max = std::max(t_max, t[7]);
        }
        for (size_t k = 0; k < idx.size(); ++k) {
            const uint64_t *t = &tm[16 * k];
            const int kind = (int)c->fl_pending[idx[k]].kind;
            s_max = std::max(s_max, t[0]); d_min = std::min(d_min, t[7] - t[0]); d_max = std::max(d_max, t[7] - t[0]);
            k_max[kind] = std::max(k_max[kind], t[7] - t[0]); k_end[kind] = std::max(k_end[kind], t[7] - t_min);
        }
        fprintf(stderr, "hvqm4_amd parse: slowest picture / last end per kind: I %.3f / %.3f  P %.3f / %.3f  B %.3f / %.3f ms\n",
                (double)k_max[0] * 1e-5, (double)k_end[0] * 1e-5, (double)k_max[1] * 1e-5, (double)k_end[1] * 1e-5,
                (double)k_max[2] * 1e-5, (double)k_end[2] * 1e-5);
        fprintf(stderr, "hvqm4_amd parse occupancy: %d workgroups per CU (runtime query)\n", hvq_parse_occupancy(256));
        fprintf(stderr, "hvqm4_amd parse timing: %zu pictures, kernel %.3f ms, first start -> last end %.3f ms, last start +%.3f ms, "
                "per picture %.3f .. %.3f ms\n",
                idx.size(), ms, (double)(t_max - t_min) * 1e-5, (double)(s_max - t_min) * 1e-5, (double)d_min * 1e-5, (double)d_max * 1e-5);
        if (const char *dump = getenv("HVQM4_AMD_PARSE_TIMING_DUMP")) {       /* raw rows of the latest batch: kind, bytes, 16 stamps (10 ns) */
            static int seq = 0;
            const std::string path = std::string(dump) + "." + std::to_string(seq++);
            if (FILE *f = seq <= 12 ? fopen(path.c_str(), "w") : nullptr) {
                for (size_t k = 0; k < idx.size(); ++k) {
                    fprintf(f, "%d %zu", (int)c->fl_pending[idx[k]].kind, (size_t)jobs_len_of(c, k));
                    for (int ph = 0; ph < 16; ++ph) fprintf(f, " %llu", (unsigned long long)(tm[16 * k + ph] ? tm[16 * k + ph] - t_min : 0ull));
                    fprintf(f, "\n");
                }
                fclose(f);
            }
        }
        for (int kind = 0; kind < 3; ++kind) {
            if (!pics[kind]) continue;
            std::vector<std::pair<double, int>> ord;
            for (int ph = 1; ph < 16; ++ph) if (cnt[kind][ph]) ord.push_back({ sum[kind][ph] / (double)cnt[kind][ph], ph });
            std::sort(ord.begin(), ord.end());
            fprintf(stderr, "  %c pictures (%zu), us since start:", "IPB"[kind], pics[kind]);
            double prev = 0;
            for (auto &o : ord) { fprintf(stderr, " %s %.0f (+%.0f) |", label[o.second], o.first, o.first - prev); prev = o.first; }
            fprintf(stderr, "\n");
        }
    }
    {
        const uint32_t retried = n_redo;
        uint64_t spins = 0;
        for (size_t k = 0; k < idx.size(); ++k) spins += res[k].pad[1];
        c->gpu_parse_retried = retried;
        if (want_timing_print) fprintf(stderr, "hvqm4_amd parse: %u of %zu pictures handed to the chains; decode wave waited %.1f rounds per picture\n",
                                       retried, idx.size(), (double)spins / (double)idx.size());
    }
    /* Overflow-symbol runs that outlast the device parser's cap (GP_SOVF_CAP symbols; the picture comes back HVQ_F_CAPPED): the
     * reference sums for as long as the stream says (h4m:654-677), and so does the HOST parser since round 5 -- bounded by the bits
     * the picture has left.  Such a picture (nothing an encoder writes; rounds 3-4 refused it) is parsed once more, here, from its
     * bitstream in the pinned arena; its blob replaces the device parser's, an I picture's nest is put where the stream's later
     * pictures look for it.  What even the host parser cannot end (a one-leaf tree outside the window) stays refused.
     * Bounded per batch (HVQ_REDO_MAX pictures, HVQ_REDO_BYTES of blobs): the re-parse runs serially on the caller's thread between a
     * batch's parse results and its first launch, and a crafted input whose pictures are ALL capped must not turn a 4 ms flush into
     * seconds for every stream of the batch -- beyond the bound a capped picture is refused as rounds 3-4 refused all of them. */
    constexpr uint32_t HVQ_REDO_MAX = 32;
    constexpr size_t HVQ_REDO_BYTES = (size_t)32 << 20;
    uint32_t n_reparsed = 0;
    c->rp_host.clear();
    for (size_t k = 0; k < idx.size(); ++k) {
        Pending &p = c->fl_pending[idx[k]];
        const size_t raw_len = jobs_len_of(c, k);
        p.status = (int)res[k].status;                 /* judged per picture by flush_end: one bad clip must not poison the batch */
        p.max_items = res[k].max_items; p.max_pairs = res[k].max_pairs;
        p.flags = res[k].flags;
        p.pool_dwords = res[k].pool_dwords;
        p.redo = false;
        if (!p.status && (p.flags & HVQ_F_CAPPED) && !p.dropped && raw_len && n_reparsed < HVQ_REDO_MAX && c->rp_host.size() < HVQ_REDO_BYTES) {
            ++n_reparsed;
            Stream &s = c->streams[(size_t)p.stream];
            const size_t bound = hvq_parser_blob_bound(s.parser), off = align_up(c->rp_host.size(), 256);
            c->rp_host.resize(off + bound + 2048);
            size_t out_len = 0;
            const int ft = p.kind == HVQ_PIC_I ? HVQ_FRAME_I : p.kind == HVQ_PIC_P ? HVQ_FRAME_P : HVQ_FRAME_B;
            const int rcp = hvq_parse_picture(s.parser, ft, c->fl_host + p.blob_off, raw_len, c->rp_host.data() + off, bound, &out_len);
            const HvqPicHeader *hd = (const HvqPicHeader *)(c->rp_host.data() + off);
            const uint32_t all_flags = hd->flags | hvq_parser_last_flags(s.parser);     /* incl. what pass 2 raised behind the header */
            if (rcp == HVQ_OK && !(all_flags & HVQ_F_CAPPED)) {
                p.redo = true; p.redo_off = off; p.redo_hd = *hd; p.redo_hd.flags = all_flags;
                out_len = align_up(out_len, 256);
                if (p.kind == HVQ_PIC_I) hvq_parser_packed_nest(s.parser, c->rp_host.data() + off + out_len);   /* behind the blob: always, not only when the blob has one */
                c->rp_host.resize(off + out_len + (p.kind == HVQ_PIC_I ? align_up(GP_ALIGN16(HVQ_NESTP_BYTES), 256) : 0));
                p.flags = all_flags; p.pool_dwords = hd->pool_dwords; p.max_items = hd->max_items; p.max_pairs = hd->max_pairs;
                p.blob_len = hd->total_bytes;
                continue;
            }
            c->rp_host.resize(off);                      /* still capped (or unparsable): refused by flush_end */
        }
        p.blob_len = res[k].total_bytes;
    }
    if (!c->rp_host.empty()) {
        if (c->rp_host.size() > c->rp_cap) {
            if (c->rp_dev) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->rp_dev)); c->rp_dev = nullptr; c->rp_cap = 0; }
            HIPCHK(hipMalloc((void **)&c->rp_dev, c->rp_host.size() * 2));
            c->rp_cap = c->rp_host.size() * 2;
        }
        { int rcu = staged_upload(c, c->fl_arena_id, 4, c->rp_dev, c->rp_host.data(), c->rp_host.size()); if (rcu) return rcu; }
        for (size_t k = 0; k < idx.size(); ++k) {
            const Pending &p = c->fl_pending[idx[k]];
            if (p.redo && p.kind == HVQ_PIC_I && p.dev_nest)
                HIPCHK(hipMemcpyAsync((void *)(uintptr_t)p.dev_nest, c->rp_dev + p.redo_off + align_up(p.redo_hd.total_bytes, 256),
                                      GP_ALIGN16(HVQ_NESTP_BYTES), hipMemcpyDeviceToDevice, c->stream));
        }
    }
    return HVQ_OK;
}

/* The launches of the resident batch go out launch group by launch group, inside a group dependency level by dependency level, every
 * launch on the queue build_tiles dealt its streams to (one queue, or two for large uniform batches: see there).
 * The second launch queue forks from the main stream (everything queued there so far is done before its first launch) ... */
static int queues_fork(HvqContext *c, bool *two)
{
    int nq = 1;
    for (auto &L : c->launches) nq = std::max(nq, L.queue + 1);
    *two = nq > 1;
    if (!*two) return HVQ_OK;
    if (!c->ev_fork) HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_fork, c->stream));
    for (int q = 1; q < nq; ++q) {
        if (!c->qstream[q]) {
            /* at the launch streams' priority level (hvq_context_create): a hardware queue of its own */
            int lo = 0, hi = 0;
            static const bool prio = !(getenv("HVQM4_AMD_STREAM_PRIORITY") && atoi(getenv("HVQM4_AMD_STREAM_PRIORITY")) == 0);
            if (prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo)
                HIPCHK(hipStreamCreateWithPriority(&c->qstream[q], hipStreamNonBlocking, hi));
            else HIPCHK(hipStreamCreateWithFlags(&c->qstream[q], hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&c->ev_join[q], hipEventDisableTiming));
        }
        HIPCHK(hipStreamWaitEvent(c->qstream[q], c->ev_fork, 0));
    }
    return HVQ_OK;
}

/* ... and joins it again: whatever is queued on the main stream next runs behind both queues */
static int queues_join(HvqContext *c, bool two)
{
    if (!two) return HVQ_OK;
    int nq = 1;
    for (auto &L : c->launches) nq = std::max(nq, L.queue + 1);
    for (int q = 1; q < nq; ++q) {
        HIPCHK(hipEventRecord(c->ev_join[q], c->qstream[q]));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join[q], 0));
    }
    return HVQ_OK;
}

/* one pass over the launches of the resident batch, every launch on its queue (between queues_fork and queues_join) */
static int run_launches(HvqContext *c)
{
    for (auto &L : c->launches) {
        hipStream_t st = L.queue ? c->qstream[L.queue] : c->stream;
        HIPCHK(hvq_launch_recon_inline(c->jobs_dev + L.first_tile, L.ntiles, L.max_tiles, L.tpw, L.items_cap, L.pair_cap, L.pool_cap, st));
        for (const SelfRef &sr : c->selfrefs) {
            if (sr.launch != (int)(&L - c->launches.data())) continue;
            if (sr.old_host) HIPCHK(hipMemcpyAsync(sr.dst, sr.old_host, sr.pic_bytes, hipMemcpyHostToDevice, st));
            else if (sr.old_dev) HIPCHK(hipMemcpyAsync(sr.dst, sr.old_dev, sr.pic_bytes, hipMemcpyDeviceToDevice, st));
            HIPCHK(hvq_launch_selfref(c->jobs_dev + sr.job, c->selfref_dev + sr.side_off, sr.dst, st));
        }
    }
    return HVQ_OK;
}

/* launch table of the batch in flight: one launch per launch group, dependency level and queue, one slot {job, tiles} per picture;
 * the slot count of a launch is padded to a multiple of 8 so that grid column x runs on XCD x % 8 and a picture's tiles share one L2.
 * The launches are pushed -- and later issued (run_launches) -- group by group, inside a group level by level, inside a level queue
 * by queue: a stream belongs to one group and one queue, so its pictures stay in level order on one in-order queue, which is all
 * their dependencies need (clips are independent).  A batch within the context's group budget is one group: level-major over all
 * its streams, as before there were groups.  The queues are forked and joined once around all groups (flush_end, replay_passes).
 * Needs nothing from the GPU, so it is built and uploaded while the parse kernel runs. */
static int build_tiles(HvqContext *c)
{
    std::vector<HvqTileRef> &tiles = c->tiles_host;
    tiles.clear();
    c->fl_launches.clear();
    int max_level = 0;
    for (auto &p : c->fl_pending) max_level = std::max(max_level, p.level);
    /* Two launch queues: clips are independent, so the dependency levels of two halves of the streams form two chains of launches
     * that run on two HIP streams with a hardware queue each -- while one chain drains a level or waits at the head of the next, the
     * other keeps the CUs busy (a launch is some twenty generations of workgroups; the first and the last of them leave CUs idle).
     * Rounds 1-4 had this behind HVQM4_AMD_QUEUES and dropped it (-7 ... -9 %): the second stream was a plain one, and the runtime deals
     * plain streams to four hardware queues in creation order -- with the context's copy and read-back streams in between, the two
     * launch streams could share one.  At the launch streams' own priority level: dense 965 -> 900 us per step (tools/replay_pair_probe.py,
     * profiles/r05_flush_next.txt 7); 64 / 32 / 16 streams gain 7 / 14 / 19 %.  Batches of fewer than 16 streams keep one queue (each queue's
     * launches should hold the 8 picture slots that spread a launch over the XCDs); HVQM4_AMD_QUEUES=1 / 2 forces either. */
    int nq = 1;
    {
        static const int qenv = getenv("HVQM4_AMD_QUEUES") ? atoi(getenv("HVQM4_AMD_QUEUES")) : 0;
        std::vector<char> seen(c->streams.size(), 0);
        size_t nstreams = 0;
        bool uniform = true;                               /* every picture of the batch has the same number of tiles */
        for (auto &p : c->fl_pending) {
            if (!seen[(size_t)p.stream]) { seen[(size_t)p.stream] = 1; ++nstreams; }
            uniform &= p.ntiles == c->fl_pending[0].ntiles;
        }
        /* mixed picture sizes keep one queue: BASELINE config 4 (320x240 and 640x480 clips alternating, 25 levels) took 1762 us per step
         * with two queues against 1303 with one, however the streams were dealt (a launch's grid is as tall as its largest picture) */
        nq = qenv >= 2 ? std::min(qenv, 4) : (qenv == 1 ? 1 : (c->max_queues >= 2 && nstreams >= 16 && uniform ? 2 : 1));
        /* streams to queues by WORK (tiles of their pictures in this batch), heaviest first to the lighter queue: clips of mixed sizes
         * (BASELINE config 4 alternates 320x240 and 640x480) dealt by parity put every large clip on one queue, and that chain then ran
         * alone for most of the step (1766 against 1295 us) */
        /* Launch groups: level-major over a large batch, everything the batch touches at two levels (0.7 GB for 128 dense streams of
         * 640x480) passes between an anchor's write and its reads, several times the 256 MiB last-level cache.  The streams of a
         * group walk all their levels before the next group starts, so that window is the group's (hvq_launch_group_plan: the rule,
         * in bytes; profiles/r10_launch_groups.txt: what it measured).  HVQM4_AMD_GROUP_BYTES overrides the context's budget. */
        static const char *genv = getenv("HVQM4_AMD_GROUP_BYTES");
        const uint64_t budget = genv ? strtoull(genv, nullptr, 10) : c->group_bytes;
        std::vector<uint32_t> ids, pic_bytes, first;
        std::vector<uint32_t> dense(c->streams.size(), 0);
        for (size_t sidx = 0; sidx < seen.size(); ++sidx)
            if (seen[sidx]) { dense[sidx] = (uint32_t)ids.size(); ids.push_back((uint32_t)sidx); pic_bytes.push_back(c->streams[sidx].pic_bytes); }
        first.assign(ids.size() + 1, 0);
        for (auto &p : c->fl_pending) ++first[dense[(size_t)p.stream] + 1];
        for (size_t k = 0; k < ids.size(); ++k) first[k + 1] += first[k];
        std::vector<uint8_t> kinds(c->fl_pending.size());
        std::vector<int32_t> levels(c->fl_pending.size());
        {
            std::vector<uint32_t> at(first.begin(), first.end() - 1);
            for (auto &p : c->fl_pending) { const uint32_t k = at[dense[(size_t)p.stream]]++; kinds[k] = (uint8_t)p.kind; levels[k] = p.level; }
        }
        std::vector<uint16_t> gof(ids.size(), 0);
        c->fl_groups = hvq_launch_group_plan((uint32_t)ids.size(), pic_bytes.data(), first.data(), kinds.data(), levels.data(), budget, (uint32_t)nq,
                                             gof.data(), nullptr);
        c->fl_gof.assign(c->streams.size(), 0);
        for (size_t k = 0; k < ids.size(); ++k) c->fl_gof[ids[k]] = gof[k];
        c->fl_qof.assign(c->streams.size(), 0);
        if (nq >= 2) {
            std::vector<uint64_t> work(c->streams.size(), 0);
            for (auto &p : c->fl_pending) work[(size_t)p.stream] += p.ntiles;
            std::vector<uint32_t> order;
            for (size_t sidx = 0; sidx < work.size(); ++sidx) if (seen[sidx]) order.push_back((uint32_t)sidx);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return work[a] > work[b]; });
            std::vector<uint64_t> load((size_t)c->fl_groups * 4, 0);       /* per group: its streams to the queues as the whole batch's were */
            for (uint32_t sidx : order) {
                uint64_t *ld = load.data() + (size_t)c->fl_gof[sidx] * 4;
                int q = 0;
                for (int k = 1; k < nq; ++k) if (ld[k] < ld[q]) q = k;
                c->fl_qof[sidx] = (uint8_t)q; ld[q] += work[sidx];
            }
        }
    }
    /* group -> level -> queue: every queue runs group 0's levels in order, then group 1's, and both walk the groups in the same order.
     * Nothing joins the queues between groups: a group's small I level overlaps the tail of the group before it. */
    for (int grp = 0; grp < (int)c->fl_groups; ++grp)
    for (int lvl = 0; lvl <= max_level; ++lvl)
      for (int qi = 0; qi < nq; ++qi) {
        Launch L{};
        L.queue = qi;
        L.group = grp;
        L.level = lvl; L.first_tile = (uint32_t)tiles.size();
        /* submission order (sorting same-stream pictures into one grid column of consecutive groups was tried: +1 % dense, -3 % flat, dropped) */
        /* (walking odd levels in reverse order, so that a level reads first the anchors its predecessor wrote last, was measured in
         * round 5: dense -1.5 %, flat -3 %, profiles/r05_recon_steps.txt) */
        for (size_t i = 0; i < c->fl_pending.size(); ++i) {
            const Pending &p = c->fl_pending[i];
            if (p.level != lvl || (nq >= 2 && c->fl_qof[(size_t)p.stream] != qi) || (int)c->fl_gof[(size_t)p.stream] != grp) continue;
            tiles.push_back(HvqTileRef{ (uint32_t)i, p.ntiles });
            L.max_wg[0] = std::max(L.max_wg[0], p.ntiles); L.wgs[0] += p.ntiles;
            L.max_wg[1] = std::max(L.max_wg[1], p.nwg); L.wgs[1] += p.nwg;
        }
        L.ntiles = (uint32_t)tiles.size() - L.first_tile;
        if (!L.ntiles) continue;
        if (L.ntiles >= 8)
            while (L.ntiles & 7u) { tiles.push_back(HvqTileRef{ 0xFFFFFFFFu, 0u }); ++L.ntiles; }   /* padding slots exit at once */
        c->fl_launches.push_back(L);
    }
    return HVQ_OK;                     /* the slots become the ORDER of the job table (flush_end): a workgroup finds its job by its grid position */
}

/* First half of a flush: everything that can be queued without waiting for the GPU.  The pending batch becomes the
 * batch in flight; the caller may queue the NEXT batch (hvq_submit_*) before hvq_flush_end -- its bitstreams are copied
 * and uploaded (other arena, copy stream) while this batch is being parsed. */
/* begin, part A: the queued batch's bitstreams go up (what the early uploads left); its parse kernel is queued behind them
 * (device_parse_launch) */
static int begin_upload(HvqContext *c)
{
    /* the pinned staging of this arena id is free again (hvq_flush_next knows that without asking: arena_idle) */
    if (!c->arena_idle[c->arena_id]) HIPCHK(hipEventSynchronize(c->ev_arena_free[c->arena_id]));
    /* 1. descriptors / bitstreams -> HBM; the compute stream waits for the copy stream */
    { int rc = arena_upload(c, c->arena_used); if (rc) return rc; }
    HIPCHK(hipEventRecord(c->ev_copy, c->copy_stream));
    HIPCHK(hipEventRecord(c->ev_h2d[c->arena_id], c->copy_stream));           /* the host may write this arena again behind this (arena_host_wait) */
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_copy, 0));
    return HVQ_OK;
}

/* begin, part B: the queued batch becomes the batch in flight */
static int begin_rest(HvqContext *c, int rc)
{
    /* the nest a GPU-parsed P/B picture uses: its batch's governing I picture, else the stream's kept one; the last I
     * picture of every stream is committed to the other kept slot at the end of the batch */
    c->fl_nest_pairs.clear();
    c->fl_nest_streams.clear();
    for (auto &p : c->pending)
        if (p.dev) {
            const Stream &s = c->streams[(size_t)p.stream];
            p.nest_ptr = p.nest_ref >= 0 ? c->pending[(size_t)p.nest_ref].dev_nest : (uint64_t)(uintptr_t)s.nest_keep_ptr(s.nest_cur);
        }
    for (auto &s : c->streams)
        if (s.open && s.nest_src >= 0) {
            c->fl_nest_pairs.push_back(c->pending[(size_t)s.nest_src].dev_nest);
            c->fl_nest_pairs.push_back((uint64_t)(uintptr_t)s.nest_keep_ptr(s.nest_cur ^ 1));   /* replays of this batch keep reading [nest_cur] */
            c->fl_nest_streams.push_back((int)(&s - c->streams.data()));
            s.nest_cur ^= 1;
            s.nest_src = -1;
        }
    /* the batch is in flight: levels restart from zero for whatever is queued next, which goes to the other arena */
    c->fl_pending.swap(c->pending);
    c->pending.clear();
    for (auto &p : c->fl_pending) {
        Stream &s = c->streams[(size_t)p.stream];
        s.inflight_from = std::min(s.inflight_from, p.ordinal);
    }
    for (auto &s : c->streams)
        for (auto &sl : s.slots) { sl.w_level = -1; sl.r_level = -1; }
    c->fl_host = c->host_arena; c->fl_dev = c->dev_arena; c->fl_arena_id = c->arena_id;
    c->arena_idle[c->arena_id] = false;
    std::swap(c->host_arena, c->host_arena_alt);
    std::swap(c->dev_arena, c->dev_arena_alt);
    std::swap(c->arena_cap, c->arena_cap_alt);
    c->arena_id ^= 1;
    c->arena_used = 0; c->arena_uploaded = 0; c->arena_waited = false; c->arena_host_ready = false;
    c->resv_active = false;            /* a reservation that was never submitted goes with its arena */
    c->fl_active = true;
    if (!rc) rc = build_tiles(c);
    if (rc) return flush_abandon(c, rc);
    return HVQ_OK;
}

/* First half of a flush: everything that can be queued without waiting for the GPU.  The pending batch becomes the
 * batch in flight; the caller may queue the NEXT batch (hvq_submit_*) before hvq_flush_end -- its bitstreams are copied
 * and uploaded (other arena, copy stream) while this batch is being parsed. */
HVQ_EXPORT int hvq_flush_begin(HvqContext *c)
{
    if (!c) return fail(HVQ_E_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    { int rc = flush_end(c); if (rc) return rc; }            /* at most one batch in flight */
    { int rcj = copy_join(c); if (rcj) return rcj; }         /* the queued batch's bitstreams are in the arena (streaming: copied by a worker) */
    if (c->pending.empty()) return HVQ_OK;
    const double tb0 = now_ms();
    { int rc = begin_upload(c); if (rc) return rc; }
    /* 1b. streams parsed on the GPU: bitstreams -> blobs, one launch */
    int rc = device_parse_launch(c);
    rc = begin_rest(c, rc);
    if (flush_timing()) fprintf(stderr, "flush_begin %.3f -> %.3f ms\n", tb0, now_ms());
    return rc;
}

/* Streaming step: end the batch in flight (k) and begin the queued one (k + 1) -- in the order that keeps the GPU busy.  The plain
 * pair hvq_flush_end / hvq_flush_begin leaves the GPU idle between the parse kernel of batch k and its first reconstruction launch
 * for as long as the host takes over the parse results and the job table (0.13-0.3 ms of a 4 ms period, measured); here the parse
 * kernel of batch k + 1 is queued FIRST, on its own set of buffers, so the host's part of batch k runs beside it and the launches of
 * batch k line up behind it.  Taken only when it is safe and useful: both batches parsed on the GPU throughout (a host-parsed blob
 * lives in the arena until its reconstruction ends) and the queued batch's bitstreams in the arena before batch k's parse results
 * arrive; otherwise this IS hvq_flush_end followed by hvq_flush_begin.  Returns the first error of either half; the state
 * afterwards is the one the plain pair leaves. */
HVQ_EXPORT int hvq_flush_next(HvqContext *c)
{
    if (!c) return fail(HVQ_E_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    static const bool allow = !(getenv("HVQM4_AMD_FLUSH_NEXT") && atoi(getenv("HVQM4_AMD_FLUSH_NEXT")) == 0);
    bool ahead = allow && c->fl_active && !c->pending.empty() && !PS(c).fl_idx.empty();
    if (ahead) {
        for (auto &p : c->fl_pending) if (!p.dev) { ahead = false; break; }
        for (auto &p : c->pending) if (!p.dev) { ahead = false; break; }
    }
    if (ahead && c->copy_active) {
        /* whichever comes first: the queued batch's bitstreams are in the arena (go ahead), or batch k's parse results are there
         * (its launches must not wait for a slow copy: plain order) */
        for (;;) {
            if (c->copy_done.load(std::memory_order_acquire)) break;
            if (hipEventQuery(PS(c).ev_parse) != hipErrorNotReady) { ahead = false; break; }
            for (int k = 0; k < 32; ++k) cpu_relax();
        }
    }
    if (!ahead) {
        if (flush_timing()) fprintf(stderr, "flush_next  %.3f: plain order\n", now_ms());
        const int rc_end = flush_end(c);
        const int rc_begin = hvq_flush_begin(c);
        return rc_end ? rc_end : rc_begin;
    }
    { int rcj = copy_join(c); if (rcj) { const int rc_end = flush_end(c); return rc_end ? rc_end : rcj; } }
    const double tb0 = now_ms();
    const int fl_arena = c->fl_arena_id;
    /* Everything stays on the one launch stream: parse k + 1, then the launches of batch k, in that order.  The parse kernel on a
     * stream of its own, so that the reconstruction of batch k runs BESIDE it, was built and measured (profiles/r05_flush_next.txt):
     * both kernels are bound by instruction issue, whichever reaches the CUs first keeps the other out until its workgroups thin
     * out, periods alternate 3.45 / 4.9 ms and their mean (4.17) is worse than this order's 3.94. */
    { int rcu = begin_upload(c); if (rcu) { const int rc_end = flush_end(c); return rc_end ? rc_end : rcu; } }   /* the queued batch stays queued */
    c->ps_live ^= 1;                   /* batch k + 1 parses into the other set ... */
    const int rc_parse = device_parse_launch(c);
    c->ps_live ^= 1;                   /* ... while batch k is finished from its own */
    c->abandoned = false;
    const int rc_end = flush_end(c);
    /* every GPU reader of batch k's arena is done (its parse results were taken, a second parse launch was waited for), and what
     * its staging buffers still feed is consumed before the host writes them again (behind the parse of the batch after next) */
    if (!c->abandoned) c->arena_idle[fl_arena] = true;
    c->ps_live ^= 1;
    const int rc_begin = begin_rest(c, rc_parse);
    if (flush_timing()) fprintf(stderr, "flush_next  %.3f -> %.3f ms\n", tb0, now_ms());
    return rc_end ? rc_end : rc_begin;
}

/* a flush that fails half way: the pictures of the batch in flight were never reconstructed -- they must not read as resident
 * (hvq_read_pictures / hvq_picture_device_ptr would otherwise hand out whatever their slots held), and nothing is in flight */
static int flush_abandon(HvqContext *c, int rc)
{
    for (auto &p : c->fl_pending) {
        Stream &s = c->streams[(size_t)p.stream];
        if ((size_t)p.ordinal < s.pic_slot.size() && s.pic_slot[(size_t)p.ordinal] == p.dst) {
            s.pic_slot[(size_t)p.ordinal] = -1;
            if (p.dst >= 0 && s.slots[(size_t)p.dst].pic == p.ordinal) s.slots[(size_t)p.dst].pic = -1;
        }
        s.anchor_old = s.anchor_new = -1;          /* the stream's references are gone with them: it resumes at its next I picture */
        s.need_I = true;
    }
    for (auto &s : c->streams) s.inflight_from = 0x7FFFFFFF;
    c->fl_active = false;
    c->abandoned = true;
    c->fl_pending.clear();
    PS(c).fl_idx.clear();
    c->launches.clear();                           /* nothing coherent to replay */
    return rc;
}
#define HIPCHK_FL(expr)                                                                                              \
    do {                                                                                                             \
        hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess) return flush_abandon(c, fail(HVQ_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)));      \
    } while (0)

/* Second half: take the parse results, build the job and tile tables, launch the reconstruction. */
static int flush_end(HvqContext *c)
{
    if (!c->fl_active) return HVQ_OK;
    c->fl_active = false;
    const double te0 = now_ms();
    { int rc = device_parse_finish(c); if (rc) return flush_abandon(c, rc); }
    const double te1 = now_ms();
    /* Judge the GPU-parsed pictures one by one.  A picture the parser could not take (status) or that this back end refuses
     * (unsupported_reason) is dropped together with every later picture of ITS stream in the batch; all other streams are
     * reconstructed as if it had not been there.  The dropped pictures read as "not resident", the stream waits for its next
     * I picture, and the flush reports the first such error after everything else has been launched. */
    int first_rc = HVQ_OK;
    uint32_t n_dropped = 0;
    {
        std::vector<char> broken(c->streams.size(), 0);
        for (size_t i = 0; i < c->fl_pending.size(); ++i) {
            Pending &p = c->fl_pending[i];
            Stream &s = c->streams[(size_t)p.stream];
            const char *why = nullptr;
            int code = HVQ_OK;
            if ((!broken[(size_t)p.stream] || p.kind == HVQ_PIC_I) && !p.dropped && p.dev) {
                if (p.status == (int)GP_ST_BADTREE) {       /* what the host parser flags HVQ_F_MALFORMED: the same refusal on both parse paths */
                    code = HVQ_E_UNSUPPORTED; why = unsupported_reason(HVQ_F_MALFORMED);
                }
                else if (p.status) { code = (p.status & GP_ST_OVERFLOW) ? HVQ_E_OVERFLOW : HVQ_E_ARG; why = "the GPU parser rejected the bitstream"; }
                else if ((why = unsupported_reason(p.flags)) != nullptr) code = HVQ_E_UNSUPPORTED;
            }
            if (!broken[(size_t)p.stream] && !p.dropped && !code && p.kind == HVQ_PIC_P && p.old_slot == -2 && !p.host_old) {
                const uint32_t fl = p.dev ? p.flags : ((const HvqPicHeader *)(c->fl_host + p.blob_off))->flags;
                if (fl & HVQ_F_SELF_REF) {
                    code = HVQ_E_UNSUPPORTED;
                    why = "P picture with future-referencing macroblocks (h4m:2058-2061) whose `present` buffer content -- the picture "
                          "the reference player's third buffer holds at this point -- is no longer resident: open the stream with more slots";
                }
            }
            if (code) {
                broken[(size_t)p.stream] = 1;
                if (!first_rc) first_rc = fail(code, "stream %d picture %d: %s (status %d); dropped with the later pictures of this stream, "
                                               "the other streams of the batch were decoded", p.stream, p.ordinal, why, p.status);
            }
            if (p.kind == HVQ_PIC_I && !code) broken[(size_t)p.stream] = 0;     /* an I picture restarts its stream inside the batch */
            /* dropped: follows a rejected picture of its stream in this batch, or was marked when the batch before this one was
             * judged (streaming: it was queued already).  Either way it is not reconstructed and must not read as resident. */
            if (!broken[(size_t)p.stream] && !p.dropped) continue;
            p.dropped = true;
            ++n_dropped;
            if ((size_t)p.ordinal < s.pic_slot.size() && s.pic_slot[(size_t)p.ordinal] == p.dst) {
                s.pic_slot[(size_t)p.ordinal] = -1;
                if (s.slots[(size_t)p.dst].pic == p.ordinal) s.slots[(size_t)p.dst].pic = -1;
            }
        }
        for (size_t sid = 0; sid < broken.size(); ++sid)
            if (broken[sid]) {
                Stream &s = c->streams[sid];
                /* what is already queued for the next batch follows the rejected picture: P/B pictures up to the first queued
                 * I picture are dropped; with an I picture queued the stream has restarted there and keeps its state */
                bool restarted = false;
                for (auto &q : c->pending) {
                    if (q.stream != (int)sid) continue;
                    if (q.kind == HVQ_PIC_I) { restarted = true; break; }
                    q.dropped = true;
                }
                if (!restarted) { s.anchor_old = s.anchor_new = -1; s.need_I = true; }
            }
        /* nests of broken streams are not committed (their last I picture may be among the dropped) */
        std::vector<uint64_t> keep;
        for (size_t k = 0; k < c->fl_nest_streams.size(); ++k)
            if (!broken[(size_t)c->fl_nest_streams[k]]) { keep.push_back(c->fl_nest_pairs[2 * k]); keep.push_back(c->fl_nest_pairs[2 * k + 1]); }
        c->fl_nest_pairs.swap(keep);
    }
    /* 2. job table (the tile table went up at begin) */
    std::vector<HvqJob> &jobs = c->jobs_host;
    const std::vector<HvqTileRef> &slots = c->tiles_host;          /* launch slots in launch order (build_tiles) */
    jobs.assign(slots.size(), HvqJob{});
    std::vector<size_t> tq_off(slots.size(), 0);
    std::vector<char> has_tq(slots.size(), 0);
    std::vector<uint32_t> slot_of(c->fl_pending.size(), 0);
    size_t tq_bytes = 0, side_bytes = 0;
    c->selfrefs.clear();
    HvqStats st{};
    for (size_t k = 0; k < slots.size(); ++k) {
        HvqJob &j = jobs[k];                                        /* zeroed by the assign above */
        if (slots[k].job == 0xFFFFFFFFu) continue;                  /* padding slot: total_tiles = 0, its workgroups exit at once */
        const size_t i = slots[k].job;
        slot_of[i] = (uint32_t)k;
        const Pending &p = c->fl_pending[i];
        const Stream &s = c->streams[(size_t)p.stream];
        HvqPicHeader hdev;
        if (p.dev && !p.redo) {                        /* geometry from the stream, per-picture fields from the parse result */
            hdev = s.layout;
            hdev.pic_kind = (uint8_t)p.kind; hdev.unk_shift = (uint8_t)p.unk_shift; hdev.flags = p.flags;
            if (p.kind == HVQ_PIC_I) hdev.mv_off = 0;
            hdev.nest_off = 1;
        }
        /* a GPU-parsed picture that was parsed again on the host (device_parse_finish): the host parser's blob and header */
        const HvqPicHeader *hd = p.redo ? &p.redo_hd : p.dev ? &hdev : (const HvqPicHeader *)(c->fl_host + p.blob_off);
        const uint64_t blob = p.redo ? (uint64_t)(uintptr_t)(c->rp_dev + p.redo_off) : p.dev ? p.dev_blob : (uint64_t)(uintptr_t)(c->fl_dev + p.blob_off);
        const uint64_t dst = (uint64_t)(uintptr_t)s.slot_ptr(p.dst);
        j.ring = (uint64_t)(uintptr_t)s.dev;                 /* every reference read is ring + a 32-bit offset */
        j.ref0_off = (uint32_t)(s.slot_ptr(p.ref0) - s.dev);
        j.ref1_off = (uint32_t)(s.slot_ptr(p.ref1) - s.dev);
        j.pool = blob + hd->pool_off;
        j.mv = blob + hd->mv_off;
        j.wave_base = blob + hd->wave_base_off;
        j.nest = hd->nest_off ? blob + hd->nest_off : 0;
        if (p.dev) j.nest = p.nest_ptr;
        j.slot_bytes = s.slot_bytes;
        j.flags = (hd->flags & 0xFFFFu) | ((uint32_t)hd->pic_kind << HVQ_JOB_KIND_SHIFT) | ((uint32_t)hd->unk_shift << HVQ_JOB_UNK_SHIFT);
        j.width = hd->width;
        j.mcb_w = hd->mcb_w;
        j.pool_dwords = (p.dev && !p.redo) ? p.pool_dwords : hd->pool_dwords;
        j.total_tiles = p.dropped ? 0u : hd->tile_first[3];          /* 0: the tile records of this picture become padding entries */
        if (p.dropped) continue;
        if (p.kind == HVQ_PIC_P && (hd->flags & HVQ_F_SELF_REF)) {
            /* a self-referencing P picture: the data-parallel pass writes a side buffer and leaves every block's pool offset in a
             * section of `tq_dev`; the walk behind this level's launch (hvq_selfref_kernel) merges the side buffer into the slot */
            const uint32_t nt = hd->tile_first[3];
            tq_bytes = align_up(tq_bytes, 256);
            tq_off[k] = tq_bytes;
            has_tq[k] = 1;
            j.q_offs_off = 16;
            tq_bytes += 16 + (size_t)nt * HVQ_TILE_BLOCKS * 4;
            SelfRef sr{};
            sr.job = (uint32_t)k;                        /* sr.launch: below, when the launches are known */
            sr.old_host = p.host_old;
            sr.old_dev = (p.host_old || p.old_slot == p.dst) ? nullptr : s.slot_ptr(p.old_slot);     /* -1: the zero slot */
            sr.dst = s.slot_ptr(p.dst);
            side_bytes = align_up(side_bytes, 256);
            sr.side_off = side_bytes;
            sr.pic_bytes = s.pic_bytes;
            side_bytes += s.slot_bytes;
            c->selfrefs.push_back(sr);
        }
        for (int k = 0; k < 3; ++k) {
            HvqPlaneRec &r = j.plane[k];
            r.map = blob + hd->map_off[k];
            r.dst = dst + hd->plane_off[k];
            r.plane_off = hd->plane_off[k];
            r.tile_first = hd->tile_first[k];
            const uint32_t ws = k ? hd->wshift : 0, hs = k ? hd->hshift : 0;
            r.hbvb = (uint32_t)hd->hb[k] | ((uint32_t)hd->vb[k] << 16);
            r.pw_sub = (uint32_t)(hd->width >> ws) | (ws << 16) | (hs << 24);
            if (k) j.tile_first12[k - 1] = hd->tile_first[k];
            j.hb_magic[k] = hd->hb[k] > 1 ? (uint32_t)(0x100000000ull / hd->hb[k]) + 1u : 0u;
            j.hb_magic16[k] = hd->hb[k] ? (65536u + hd->hb[k] - 1u) / hd->hb[k] : 0u;
        }
        st.pictures++;
        st.luma_pixels += (uint64_t)p.w * p.h;
        st.algorithmic_bytes += (uint64_t)s.pic_bytes * (p.kind == HVQ_PIC_I ? 1u : 2u);
        st.descriptor_bytes += p.blob_len;
        st.flags_or |= hd->flags;
        st.gpu_parsed += p.dev ? 1u : 0u;
    }
    /* LDS sizes of the launches (their tile ranges were dealt at begin): accumulators are 16 dwords per queued block,
     * rows padded to 32 entries (LDS banks); pairs above the cap take the kernel's serial fallback */
    /* fullest tile per launch: one pass over the pictures (this runs between the parse results and the first launch: the GPU waits) */
    std::vector<uint32_t> lmi(c->fl_launches.size(), 0), lmp(c->fl_launches.size(), 0);
    bool twoq = false;
    int nqs = 1;
    for (auto &L : c->fl_launches) { twoq |= L.queue >= 1; nqs = std::max(nqs, L.queue + 1); }
    /* a picture's launch: the one of its stream's group and queue at its level */
    int nlv = 1;
    for (auto &L : c->fl_launches) nlv = std::max(nlv, L.level + 1);
    std::vector<int> lidx((size_t)c->fl_groups * nlv * nqs, -1);
    for (size_t l = 0; l < c->fl_launches.size(); ++l) {
        const Launch &L = c->fl_launches[l];
        lidx[((size_t)L.group * nlv + L.level) * nqs + L.queue] = (int)l;
    }
    auto launch_of = [&](const Pending &p) -> int {
        const int q = twoq ? (int)c->fl_qof[(size_t)p.stream] : 0;
        return p.level < nlv ? lidx[((size_t)c->fl_gof[(size_t)p.stream] * nlv + p.level) * nqs + q] : -1;
    };
    for (auto &sr : c->selfrefs) sr.launch = launch_of(c->fl_pending[slots[sr.job].job]);
    for (size_t i = 0; i < c->fl_pending.size(); ++i) {
        const Pending &p = c->fl_pending[i];
        if (p.dropped) continue;
        const int l = launch_of(p);
        if (l >= 0) { lmi[(size_t)l] = std::max(lmi[(size_t)l], p.max_items); lmp[(size_t)l] = std::max(lmp[(size_t)l], p.max_pairs); }
    }
    for (size_t li = 0; li < c->fl_launches.size(); ++li) {
        Launch &L = c->fl_launches[li];
        const uint32_t mi = lmi[li], mp = lmp[li];
        static const int force_tpw = getenv("HVQM4_AMD_TILES_PER_WG") ? atoi(getenv("HVQM4_AMD_TILES_PER_WG")) : 0;
        uint32_t lds = 0;
        hvq_recon_inline_plan(mi, mp, force_tpw, &L.tpw, &L.items_cap, &L.pair_cap, &L.pool_cap, &lds);
        if (flush_timing())
            fprintf(stderr, "[flush] launch %zu (level %d, queue %d): fullest tile %u items, %u pairs -> %u tile(s) per workgroup, items %u, pairs %u, pool %u, %u B of LDS = %u workgroups per CU\n",
                    li, (int)L.level, (int)L.queue, mi, mp, L.tpw, L.items_cap, L.pair_cap, L.pool_cap, lds, hvq_recon_inline_residency(L.tpw, L.items_cap, lds));
        if (flush_timing()) fprintf(stderr, "[flush] group %d of %u: launch %zu (level %d, queue %d), %u picture slots\n", L.group, c->fl_groups, li, L.level, L.queue, L.ntiles);
        L.max_tiles = L.max_wg[L.tpw - 1]; L.workgroups = L.wgs[L.tpw - 1];
        st.workgroups += L.workgroups;
    }
    c->launches = c->fl_launches;
    c->groups = c->fl_groups;
    st.launches = (uint32_t)c->launches.size();
    st.launch_queues = (uint32_t)nqs;
    st.parse_seconds = c->parse_seconds;
    st.gpu_parse_ms = st.gpu_parsed ? c->gpu_parse_ms : 0.0;
    st.gpu_parse_retried = st.gpu_parsed ? c->gpu_parse_retried : 0u;
    st.dropped = n_dropped;
    if (jobs.size() > c->jobs_cap) {
        if (c->jobs_dev) { HIPCHK_FL(hipStreamSynchronize(c->stream)); HIPCHK_FL(hipFree(c->jobs_dev)); }
        c->jobs_cap = jobs.size() * 2;
        HIPCHK_FL(hipMalloc((void **)&c->jobs_dev, c->jobs_cap * sizeof(HvqJob)));
    }
    if (tq_bytes > c->tq_cap) {
        if (c->tq_dev) { HIPCHK_FL(hipStreamSynchronize(c->stream)); HIPCHK_FL(hipFree(c->tq_dev)); c->tq_dev = nullptr; c->tq_cap = 0; }
        const size_t ncap = align_up(tq_bytes + tq_bytes / 4, 4096);
        HIPCHK_FL(hipMalloc((void **)&c->tq_dev, ncap));
        c->tq_cap = ncap;
    }
    for (size_t k = 0; k < jobs.size(); ++k)
        if (jobs[k].total_tiles && has_tq[k]) jobs[k].tq = (uint64_t)(uintptr_t)(c->tq_dev + tq_off[k]);
    if (side_bytes > c->selfref_cap) {
        if (c->selfref_dev) { HIPCHK_FL(hipStreamSynchronize(c->stream)); HIPCHK_FL(hipFree(c->selfref_dev)); c->selfref_dev = nullptr; c->selfref_cap = 0; }
        HIPCHK_FL(hipMalloc((void **)&c->selfref_dev, side_bytes));
        c->selfref_cap = side_bytes;
    }
    for (const SelfRef &sr : c->selfrefs)
        for (int k = 0; k < 3; ++k) {
            HvqPlaneRec &r = jobs[sr.job].plane[k];
            r.dst = (uint64_t)(uintptr_t)(c->selfref_dev + sr.side_off) + r.plane_off;
        }
    /* stream-ordered after whatever still reads the previous table */
    { int rcu = staged_upload(c, c->fl_arena_id, 2, c->jobs_dev, jobs.data(), jobs.size() * sizeof(HvqJob)); if (rcu) return flush_abandon(c, rcu); }
    /* 3. one launch per level */
    {
        bool two = false;
        int rc = export_fence(c);
        if (!rc) rc = queues_fork(c, &two);
        if (!rc) rc = run_launches(c);
        /* joined also when a launch failed: whatever the other queues hold is ordered in front of everything the main stream gets next */
        { const int rcj = queues_join(c, two); if (!rc) rc = rcj; }
        if (rc) return flush_abandon(c, rc);
    }
    if (!c->fl_nest_pairs.empty()) {   /* the last I picture's nest of every GPU-parsed stream must outlive this batch's buffers */
        { int rcu = staged_upload(c, c->fl_arena_id, 3, PS(c).np_dev, c->fl_nest_pairs.data(), c->fl_nest_pairs.size() * sizeof(uint64_t)); if (rcu) return flush_abandon(c, rcu); }
        HIPCHK_FL(hvq_launch_nest_commit(PS(c).np_dev, (uint32_t)(c->fl_nest_pairs.size() / 2), c->stream));
    }
    HIPCHK_FL(hipEventRecord(c->ev_arena_free[c->fl_arena_id], c->stream));    /* this batch's arena may be refilled after this */
    HIPCHK_FL(hipEventRecord(c->ev_read, c->stream));                           /* every picture flushed so far is complete behind this */
    for (auto &s : c->streams) s.inflight_from = 0x7FFFFFFF;
    c->stats = st;
    c->fl_pending.clear();
    PS(c).fl_idx.clear();
    if (flush_timing()) fprintf(stderr, "flush_end   %.3f: parse results at %.3f, launches queued %.3f ms (parse kernel %.3f ms)\n", te0, te1, now_ms(), c->gpu_parse_ms);
    return first_rc;
}

HVQ_EXPORT int hvq_flush_end(HvqContext *c)
{
    if (!c) return fail(HVQ_E_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    return flush_end(c);
}

HVQ_EXPORT int hvq_flush(HvqContext *c)
{
    int rc = hvq_flush_begin(c);
    return rc ? rc : hvq_flush_end(c);
}

HVQ_EXPORT int hvq_sync(HvqContext *c)
{
    if (!c) return fail(HVQ_E_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    { int rcj = copy_join(c); if (rcj) return rcj; }
    { int rc = flush_end(c); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(c->stream));
    return HVQ_OK;
}

/* `reps` passes over the resident batch.  joined = true: every pass forks and joins the launch queues exactly as a flush does
 * (flush_end: queues_fork, run_launches, queues_join) -- the product's step, pass r + 1 starts when BOTH queues have finished pass r.
 * joined = false: the queues fork once and join once around all passes (inside a queue pass r + 1 follows pass r in stream order, and
 * the queues hold different streams' pictures): a queue that is ahead runs into the next pass, which hides the queues' imbalance and
 * one join per step -- measured beside the joined form, never the headline.
 * (Round 5 measured a HIP graph of the pass for small batches -- one GPU's share of BASELINE config 4, 128 pictures in 7 launches --
 * 92.4 us per step against 87.2 with plain launches, profiles/r05_recon_steps.txt.  The launches are a dependency chain, each as long as
 * a workgroup's lifetime; there is no launch overhead for a graph to remove.  Not kept.) */
static int replay_passes(HvqContext *c, bool joined, int reps)
{
    bool two = false;
    { int rc = export_fence(c); if (rc) return rc; }
    if (!joined) { int rc = queues_fork(c, &two); if (rc) return rc; }
    for (int r = 0; r < reps; ++r) {
        if (joined) { int rc = queues_fork(c, &two); if (rc) return rc; }
        { int rc = run_launches(c); if (rc) return rc; }
        if (joined) { int rc = queues_join(c, two); if (rc) return rc; }
    }
    return joined ? HVQ_OK : queues_join(c, two);
}

HVQ_EXPORT int hvq_replay(HvqContext *c, int reps, float *gpu_ms)
{
    if (!c || reps < 0) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = flush_end(c); if (rc) return rc; }
    if (c->launches.empty()) return fail(HVQ_E_STATE, "nothing flushed yet");
    if (!c->selfrefs.empty())
        return fail(HVQ_E_STATE, "the resident batch holds self-referencing P pictures: their previous buffer content is gone after the first pass");
    if (!c->pending.empty()) return fail(HVQ_E_STATE, "pictures queued since the last flush");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    { int rc = replay_passes(c, false, reps); if (rc) return rc; }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (gpu_ms) *gpu_ms = ms;
#ifdef HVQ_STAMPS
    if (getenv("HVQM4_AMD_STAMPS")) {
        /* diagnostic build: one more pass with phase stamps, per-launch mean segment lengths on stderr */
        static const char *seg_i[14] = { "job record (+ early barrier)", "trip 2 issue", "trip 2 lands", "classes, rows requested, scans", "slots, lists",
                                         "rows land", "phase A", "barrier 1", "pair phase (B1)", "barrier 2", "item phase (B2)", "barrier 3", "store issue", "stores land" };
        static const int from_i[14] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13 }, to_i[14] = { 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14 };
        for (auto &L : c->launches) {
            const char **seg = seg_i;
            const int *from = from_i, *to = to_i;
            const int NS = 14, LAST = 14;
            unsigned long long *d = nullptr;
            const size_t n = (size_t)L.ntiles * L.max_tiles * 64;
            HIPCHK(hipMalloc((void **)&d, n * 8));
            HIPCHK(hipMemsetAsync(d, 0, n * 8, c->stream));
            hvq_set_stamps(d);
            HIPCHK(hvq_launch_recon_inline(c->jobs_dev + L.first_tile, L.ntiles, L.max_tiles, L.tpw, L.items_cap, L.pair_cap, L.pool_cap, c->stream));
            hvq_set_stamps(nullptr);
            std::vector<unsigned long long> h(n);
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipMemcpy(h.data(), d, n * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipFree(d));
            double sum[14] = {}, life = 0; size_t cnt[14] = {}, nw = 0;
            for (size_t t = 0; t < (size_t)L.ntiles * L.max_tiles; ++t)
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long *q = &h[t * 64 + w * 16];
                    if (!q[LAST]) continue;
                    for (int k = 0; k < NS; ++k)
                        if (q[from[k]] && q[to[k]]) { sum[k] += (double)(q[to[k]] - q[from[k]]); cnt[k]++; }
                    life += (double)(q[LAST] - q[0]); nw++;
                }
            fprintf(stderr, "stamps L%d: %u workgroups, %zu waves, mean wave lifetime %.0f cycles;", L.level, L.workgroups, nw, nw ? life / nw : 0.0);
            for (int k = 0; k < NS; ++k) fprintf(stderr, " %s %.0f |", seg[k], cnt[k] ? sum[k] / cnt[k] : 0.0);
            fprintf(stderr, "\n");
        }
    }
#endif
    return HVQ_OK;
}

/* what = 1: `reps` passes, each forking and joining the launch queues as a flush does -- the reconstruction stage of the product,
 * everything a batch of new pictures costs behind its parse (bench.py's timed step).  what = 0: hvq_replay (the queues run free over
 * all passes).  what = 2: nothing (it timed the queue build of the two-pass variant, deleted in round 6; kept so that callers of
 * rounds 3-5 still link): 0 ms. */
HVQ_EXPORT int hvq_replay_stage(HvqContext *c, int reps, int what, float *gpu_ms)
{
    if (!c || reps < 0 || what < 0 || what > 2) return fail(HVQ_E_ARG, "bad arguments");
    if (what == 0) return hvq_replay(c, reps, gpu_ms);
    { int rc = flush_end(c); if (rc) return rc; }
    if (c->launches.empty()) return fail(HVQ_E_STATE, "nothing flushed yet");
    if (!c->selfrefs.empty())
        return fail(HVQ_E_STATE, "the resident batch holds self-referencing P pictures: their previous buffer content is gone after the first pass");
    if (!c->pending.empty()) return fail(HVQ_E_STATE, "pictures queued since the last flush");
    if (what == 2) { if (gpu_ms) *gpu_ms = 0.f; return HVQ_OK; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    { int rc = replay_passes(c, true, reps); if (rc) return rc; }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (gpu_ms) *gpu_ms = ms;
    return HVQ_OK;
}

HVQ_EXPORT int hvq_read_picture(HvqContext *c, int sid, int ordinal, void *dst, size_t cap)
{
    if (!c || sid < 0 || sid >= (int)c->streams.size() || !c->streams[sid].open) return fail(HVQ_E_ARG, "bad stream %d", sid);
    Stream &s = c->streams[sid];
    if (ordinal < 0 || ordinal >= s.npics) return fail(HVQ_E_ARG, "bad picture ordinal %d", ordinal);
    if (cap < s.pic_bytes) return fail(HVQ_E_ARG, "destination too small");
    { int rc = flush_end(c); if (rc) return rc; }
    for (auto &p : c->pending)
        if (p.stream == sid && p.ordinal == ordinal) return fail(HVQ_E_STATE, "picture %d is queued but not flushed", ordinal);
    int slot = s.pic_slot[(size_t)ordinal];
    if (slot < 0) return fail(HVQ_E_STATE, "picture %d is no longer resident (slot reused)", ordinal);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(dst, s.slot_ptr(slot), s.pic_bytes, hipMemcpyDeviceToHost));
    return HVQ_OK;
}

/* a 4:2:0 picture (Y|U|V at `yuv`) to dense RGB24: the jobs of the display epilogue */
static HvqRgbJob rgb420_job(const uint8_t *yuv, int w, int h)
{
    const size_t n = (size_t)w * h;
    return HvqRgbJob{ yuv, yuv + n, yuv + n + n / 4, nullptr, (int64_t)w * 3, 0, w, h, 1, 1 };
}

/* convert `n` 4:2:0 pictures in one launch into consecutive regions of the RGB scratch; optional timing */
static int rgb_run(HvqContext *c, HvqRgbJob *jobs, int n, int reps, float *gpu_ms)
{
    size_t need = 0;
    int max_lanes = 0, wide = 1;
    for (int i = 0; i < n; ++i) if (jobs[i].w % 16) wide = 0;
    for (int i = 0; i < n; ++i) { need += (size_t)jobs[i].w * jobs[i].h * 3; max_lanes = std::max(max_lanes, (jobs[i].w >> 2) * jobs[i].h); }
    if (need > c->rgb_cap) {
        if (c->rgb_dev) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->rgb_dev)); }
        HIPCHK(hipMalloc((void **)&c->rgb_dev, need));
        c->rgb_cap = need;
    }
    if ((size_t)n > c->rgb_jobs_cap) {
        if (c->rgb_jobs_dev) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->rgb_jobs_dev)); }
        HIPCHK(hipMalloc((void **)&c->rgb_jobs_dev, (size_t)n * sizeof(HvqRgbJob)));
        c->rgb_jobs_cap = (size_t)n;
    }
    size_t off = 0;
    for (int i = 0; i < n; ++i) { jobs[i].dst = c->rgb_dev + off; off += (size_t)jobs[i].w * jobs[i].h * 3; }
    HIPCHK(hipMemcpyAsync(c->rgb_jobs_dev, jobs, (size_t)n * sizeof(HvqRgbJob), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (gpu_ms) HIPCHK(hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < reps; ++r) HIPCHK(hvq_launch_rgb(c->rgb_jobs_dev, n, max_lanes, wide, HVQ_FMT_RGB24, c->stream));
    if (gpu_ms) {
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        HIPCHK(hipEventSynchronize(c->ev1));
        HIPCHK(hipEventElapsedTime(gpu_ms, c->ev0, c->ev1));
    }
    return HVQ_OK;
}

HVQ_EXPORT int hvq_read_picture_rgb(HvqContext *c, int sid, int ordinal, void *dst, size_t cap)
{
    if (!c || sid < 0 || sid >= (int)c->streams.size() || !c->streams[sid].open) return fail(HVQ_E_ARG, "bad stream %d", sid);
    Stream &s = c->streams[sid];
    if (ordinal < 0 || ordinal >= s.npics) return fail(HVQ_E_ARG, "bad picture ordinal %d", ordinal);
    const size_t need = (size_t)s.w * s.h * 3;
    if (cap < need) return fail(HVQ_E_ARG, "destination too small");
    if (s.pic_bytes != (uint32_t)(s.w * s.h * 3 / 2)) return fail(HVQ_E_GEOMETRY, "RGB epilogue needs 4:2:0");
    { int rc = flush_end(c); if (rc) return rc; }
    for (auto &p : c->pending)
        if (p.stream == sid && p.ordinal == ordinal) return fail(HVQ_E_STATE, "picture %d is queued but not flushed", ordinal);
    int slot = s.pic_slot[(size_t)ordinal];
    if (slot < 0) return fail(HVQ_E_STATE, "picture %d is no longer resident (slot reused)", ordinal);
    HIPCHK(hipSetDevice(c->device));
    HvqRgbJob job = rgb420_job(s.slot_ptr(slot), s.w, s.h);
    int rc = rgb_run(c, &job, 1, 1, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dst, c->rgb_dev, need, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return HVQ_OK;
}

/* the reference player's dumpRGB (h4m:897-926) on a host picture: Y|U|V 4:2:0 in, RGB24 out */
HVQ_EXPORT int hvq_convert_yuv420_rgb(HvqContext *c, const void *yuv, int width, int height, void *rgb)
{
    if (!c || !yuv || !rgb || width <= 0 || height <= 0 || (width & 3) || (height & 1) || width > 16384 || height > 16384)
        return fail(HVQ_E_ARG, "bad arguments (width a multiple of 4, height even)");
    HIPCHK(hipSetDevice(c->device));
    { int rc = flush_end(c); if (rc) return rc; }
    const size_t nyuv = (size_t)width * height * 3 / 2, nrgb = (size_t)width * height * 3;
    uint8_t *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, nyuv));
    hipError_t e = hipMemcpyAsync(d, yuv, nyuv, hipMemcpyHostToDevice, c->stream);
    int rc = HVQ_OK;
    if (e != hipSuccess) rc = fail(HVQ_E_HIP, "upload: %s", hipGetErrorString(e));
    HvqRgbJob job = rgb420_job(d, width, height);
    if (!rc) rc = rgb_run(c, &job, 1, 1, nullptr);
    if (!rc) {
        e = hipMemcpyAsync(rgb, c->rgb_dev, nrgb, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(HVQ_E_HIP, "download: %s", hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    return rc;
}

/* ---- getting pictures out at the rate they are made (the per-picture hvq_read_picture synchronises every time) ---- */
HVQ_EXPORT void *hvq_pinned_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { fail(HVQ_E_HIP, "hipHostMalloc(%zu) failed", bytes); return nullptr; }
    return p;
}

HVQ_EXPORT void hvq_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

/* resident picture -> its slot, after ending the batch in flight; nullptr + error when it is queued, unknown or gone */
static const uint8_t *resident_picture(HvqContext *c, int sid, int ordinal, int *rc)
{
    *rc = HVQ_OK;
    if (sid < 0 || sid >= (int)c->streams.size() || !c->streams[(size_t)sid].open) { *rc = fail(HVQ_E_ARG, "bad stream %d", sid); return nullptr; }
    Stream &s = c->streams[(size_t)sid];
    if (ordinal < 0 || ordinal >= s.npics) { *rc = fail(HVQ_E_ARG, "stream %d: bad picture ordinal %d", sid, ordinal); return nullptr; }
    for (auto &p : c->pending)
        if (p.stream == sid && p.ordinal == ordinal) { *rc = fail(HVQ_E_STATE, "stream %d picture %d is queued but not flushed", sid, ordinal); return nullptr; }
    const int slot = s.pic_slot[(size_t)ordinal];
    if (slot < 0) { *rc = fail(HVQ_E_STATE, "stream %d picture %d is no longer resident (slot reused, or the picture was dropped)", sid, ordinal); return nullptr; }
    return s.slot_ptr(slot);
}

/* ---- The lookup that hvq_read_pictures and every member of the export chain share ("The shared picture lookup") ---- */

/* does (sid, ordinal) belong to the batch in flight?  A stream that does not exist has no say: the lookup refuses it afterwards */
static bool in_flight(const HvqContext *c, int sid, int ordinal)
{
    return sid >= 0 && sid < (int)c->streams.size() && ordinal >= c->streams[(size_t)sid].inflight_from;
}

/* First half of a call.  Pictures of batches that hvq_flush_end has launched are used WITHOUT ending the batch in flight: a streaming
 * player calls flush_end(k), flush_begin(k + 1), read(k) -- the work on batch k then runs beside the parse of batch k + 1.  Only when
 * a requested resident picture belongs to the batch in flight is that batch ended first.  Both sides of a call are asked: picture i
 * unless the caller's memory stands in for it (`src[i]`), and reference i when it names a stream; `src` and `ref` may be NULL. */
static int chain_begin(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src, const HvqMetricsRef *ref)
{
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < n; ++i)
        if ((!(src && src[i]) && in_flight(c, streams[i], ordinals[i])) || (ref && ref[i].stream >= 0 && in_flight(c, ref[i].stream, ref[i].ordinal)))
            return flush_end(c);
    return HVQ_OK;
}

/* Picture i of a call -> *a: the caller's memory (`src[i]`: a multiple of 16, laid out as the pictures of streams[i] are, ordinal -1)
 * or the resident picture (streams[i], ordinals[i]).  Called once per picture, where the entry point's loop reaches it: the first
 * fault in picture order is the one a call reports. */
static int picture_source(HvqContext *c, int i, const int *streams, const int *ordinals, const void *const *src, const uint8_t **a)
{
    int rc = HVQ_OK;
    if (src && src[i]) {
        if (streams[i] < 0 || streams[i] >= (int)c->streams.size() || !c->streams[(size_t)streams[i]].open) return fail(HVQ_E_ARG, "bad stream %d", streams[i]);
        if (ordinals[i] != -1) return fail(HVQ_E_ARG, "picture %d: a pointer together with ordinal %d (the caller's memory takes ordinal -1)", i, ordinals[i]);
        if ((uintptr_t)src[i] & 15u) return fail(HVQ_E_ARG, "picture %d: the pointer must be a multiple of 16", i);
        *a = (const uint8_t *)src[i];
    } else {
        *a = resident_picture(c, streams[i], ordinals[i], &rc);
    }
    return rc;
}

/* Reference i of a call (`r`, NULL when the call has none) against a picture of stream `sid` -> *b: a resident picture of the same
 * geometry (r->stream >= 0, no pointer), the caller's memory (stream -1, a pointer that is a multiple of 16) or nullptr (stream -1, no
 * pointer: zeros).  A call that takes no zeros says why in `no_zeros` (NULL: zeros are a reference), and they are refused in those words. */
static int picture_reference(HvqContext *c, int i, int sid, const HvqMetricsRef *r, const char *no_zeros, const uint8_t **b)
{
    *b = nullptr;
    if (!r) return HVQ_OK;
    if (r->stream >= 0) {
        if (r->ptr) return fail(HVQ_E_ARG, "reference %d: a pointer together with stream %d (a resident reference takes no pointer)", i, r->stream);
        int rc = HVQ_OK;
        *b = resident_picture(c, r->stream, r->ordinal, &rc);
        if (!*b) return rc;
        const Stream &s = c->streams[(size_t)sid], &t = c->streams[(size_t)r->stream];
        if (t.w != s.w || t.h != s.h || t.wshift != s.wshift || t.hshift != s.hshift)
            return fail(HVQ_E_ARG, "reference %d: stream %d (%d x %d, chroma shifts %d, %d) has not the geometry of stream %d (%d x %d, %d, %d)", i,
                        r->stream, t.w, t.h, t.wshift, t.hshift, sid, s.w, s.h, s.wshift, s.hshift);
    } else if (r->stream != -1) {
        return fail(HVQ_E_ARG, "reference %d: stream %d (a stream, or -1 for the caller's memory%s)", i, r->stream, no_zeros ? "" : " or zeros");
    } else if (r->ptr) {
        if ((uintptr_t)r->ptr & 15u) return fail(HVQ_E_ARG, "reference %d: the pointer must be a multiple of 16", i);
        *b = (const uint8_t *)r->ptr;
    } else if (no_zeros) {
        return fail(HVQ_E_ARG, "reference %d: %s (stream -1 needs a pointer)", i, no_zeros);
    }
    return HVQ_OK;
}

/* The context's own scratch of one kind of call (ck_acc, jp_scr, ph_acc), reused by every such call: the chain orders the calls.  When
 * `need` elements of `elem` bytes exceed it, the chain is drained (an earlier call may still use the buffer that goes) and the buffer
 * comes back at twice the need, a multiple of `align` elements and `limit` at the most (a `limit` never below the need). */
template <class T>
static int scratch_grow(HvqContext *c, T **buf, size_t *cap, size_t need, size_t align, size_t limit = SIZE_MAX)
{
    if (need <= *cap) return HVQ_OK;
    { int rc = export_drain(c); if (rc) return rc; }
    if (*buf) { HIPCHK(hipFree(*buf)); *buf = nullptr; *cap = 0; }
    const size_t ncap = std::min(align_up(need * 2, align), limit);
    HIPCHK(hipMalloc((void **)buf, ncap * sizeof(T)));
    *cap = ncap;
    return HVQ_OK;
}

/* is this a geometry the library decodes, and so one whose pictures it handles?  (a parser's tables are the check) */
static int geometry_supported(int width, int height, int h_samp, int v_samp)
{
    HvqParser *p = hvq_parser_create(width, height, h_samp, v_samp, 1);
    if (!p) return fail(HVQ_E_GEOMETRY, "unsupported geometry %dx%d sampling %dx%d", width, height, h_samp, v_samp);
    hvq_parser_destroy(p);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_read_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, void *const *dst)
{
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = chain_begin(c, n, streams, ordinals, nullptr, nullptr); if (rc) return rc; }
    /* all copies are queued on the read stream behind the launches of the last ended batch (the event flush_end recorded); ONE
     * wait at the end */
    HIPCHK(hipStreamWaitEvent(c->read_stream, c->ev_read, 0));
    std::vector<const uint8_t *> src((size_t)n);
    bool same = n > 0;
    for (int i = 0; i < n; ++i) {
        int rc = HVQ_OK;
        src[(size_t)i] = resident_picture(c, streams[i], ordinals[i], &rc);
        if (!src[(size_t)i]) return rc;
        if (!dst[i]) return fail(HVQ_E_ARG, "null destination %d", i);
        same = same && c->streams[(size_t)streams[i]].pic_bytes == c->streams[(size_t)streams[0]].pic_bytes;
    }
    if (same && n >= 4) {
        /* every picture lives in its own slot: a kernel gathers them into one buffer (HBM speed), and what crosses PCIe is one
         * transfer per run of consecutive destinations instead of one per picture (2048 x 460 KB: 20 GB/s apiece, ~50 together) */
        const uint32_t pb = c->streams[(size_t)streams[0]].pic_bytes;
        const size_t need = (size_t)n * pb;
        if (need > c->rb_cap) {
            if (c->rb_dev) { HIPCHK(hipStreamSynchronize(c->read_stream)); HIPCHK(hipFree(c->rb_dev)); c->rb_dev = nullptr; c->rb_cap = 0; }
            HIPCHK(hipMalloc((void **)&c->rb_dev, need));
            c->rb_cap = need;
        }
        if ((size_t)n > c->rb_tab_cap) {
            HIPCHK(hipStreamSynchronize(c->read_stream));
            if (c->rb_tab_dev) HIPCHK(hipFree(c->rb_tab_dev));
            if (c->rb_tab_host) HIPCHK(hipHostFree(c->rb_tab_host));
            c->rb_tab_dev = nullptr; c->rb_tab_host = nullptr;
            c->rb_tab_cap = (size_t)n * 2;
            HIPCHK(hipMalloc((void **)&c->rb_tab_dev, c->rb_tab_cap * sizeof(uint64_t)));
            HIPCHK(hipHostMalloc((void **)&c->rb_tab_host, c->rb_tab_cap * sizeof(uint64_t), hipHostMallocDefault));
        }
        for (int i = 0; i < n; ++i) c->rb_tab_host[i] = (uint64_t)(uintptr_t)src[(size_t)i];
        HIPCHK(hipMemcpyAsync(c->rb_tab_dev, c->rb_tab_host, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->read_stream));
        HIPCHK(hvq_launch_gather(c->rb_tab_dev, c->rb_dev, (uint32_t)n, pb, c->read_stream));
        for (int i = 0; i < n;) {
            int j = i + 1;
            while (j < n && (uint8_t *)dst[j] == (uint8_t *)dst[j - 1] + pb) ++j;
            HIPCHK(hipMemcpyAsync(dst[i], c->rb_dev + (size_t)i * pb, (size_t)(j - i) * pb, hipMemcpyDeviceToHost, c->read_stream));
            i = j;
        }
    } else {
        for (int i = 0; i < n; ++i)
            HIPCHK(hipMemcpyAsync(dst[i], src[(size_t)i], c->streams[(size_t)streams[i]].pic_bytes, hipMemcpyDeviceToHost, c->read_stream));
    }
    HIPCHK(hipStreamSynchronize(c->read_stream));
    return HVQ_OK;
}

/* device address of a resident picture (Y|U|V, hvq_stream_pic_bytes) for consumers on the GPU; valid until the stream's ring
 * hands the slot to a later picture (nslots pictures later at the earliest).  Work queued by the caller must be ordered after
 * hvq_sync(), or after the event the caller records behind it. */
HVQ_EXPORT int hvq_picture_device_ptr(HvqContext *c, int sid, int ordinal, const void **ptr)
{
    if (!c || !ptr) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = flush_end(c); if (rc) return rc; }
    int rc = HVQ_OK;
    *ptr = resident_picture(c, sid, ordinal, &rc);
    return rc;
}

/* What the members of the export chain share, second half (chain_begin is the first), once everything is checked: from here on the
 * call enqueues.  The job table the export K calls ago used is free
 * once that export has run (a host wait only when K exports are still queued); `launch(table in device memory, stream)` queues the
 * kernel behind the table's upload, the reconstruction of every flushed picture and the previous export */
template <class Launch>
static int export_enqueue(HvqContext *c, const void *jobs, size_t bytes, void *hip_stream, Launch launch)
{
    HvqContext::ExportTab &T = c->ex[c->ex_next];
    if (!T.ev) HIPCHK(hipEventCreateWithFlags(&T.ev, hipEventDisableTiming));
    else if (T.used) HIPCHK(hipEventSynchronize(T.ev));
    if (bytes > T.cap) {                                      /* bytes: a multiple of 16, hvq_launch_upload copies whole 16-byte units */
        if (T.host) { HIPCHK(hipHostFree(T.host)); T.host = nullptr; }
        if (T.dev) { HIPCHK(hipFree(T.dev)); T.dev = nullptr; }
        T.cap = 0;
        const size_t ncap = align_up(bytes * 2, 4096);
        HIPCHK(hipHostMalloc((void **)&T.host, ncap, hipHostMallocDefault));
        HIPCHK(hipMalloc((void **)&T.dev, ncap));
        T.cap = ncap;
    }
    memcpy(T.host, jobs, bytes);
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCHK(hipStreamWaitEvent(st, c->ev_read, 0));                          /* every flushed picture is reconstructed */
    if (c->ex_last >= 0) HIPCHK(hipStreamWaitEvent(st, c->ex[c->ex_last].ev, 0));   /* chained: the newest export covers all */
    HIPCHK(hvq_launch_upload(T.host, T.dev, bytes, st));
    HIPCHK(launch((const void *)T.dev, st));
    HIPCHK(hipEventRecord(T.ev, st));
    T.used = true;
    c->ex_last = c->ex_next;
    c->ex_next = (c->ex_next + 1) % (int)(sizeof c->ex / sizeof c->ex[0]);
    c->ex_unfenced = true;
    return HVQ_OK;
}

/* ---- The frame of the calls that write uint8 pictures in slot layout, Y | U | V ("The slot-layout frame"): scale,
 * filter, warp, compose, rank, bilateral, map.  Everything here inlines into the entry point's loop: no allocation, no indirect call ---- */

/* "%d pictures": the most one launch's grid takes; `why` is what a record call adds to the text (GRID_ROW) */
static int count_check(int n, const char *noun, const char *why = "")
{
    if (n > 65535) return fail(HVQ_E_ARG, "%d %s: one call takes 65535 at the most%s", n, noun, why);
    return HVQ_OK;
}

/* destination (or target) i of a call: the kernels store 16 bytes at a time */
static int slot_pointer_check(const char *noun, int i, const void *ptr)
{
    if (!ptr || ((uintptr_t)ptr & 15u)) return fail(HVQ_E_ARG, "%s %d: the pointer must be a non-null multiple of 16", noun, i);
    return HVQ_OK;
}

/* A call usually repeats few target shapes: the geometry check (a parser's tables) is kept from the target before. */
struct TargetSeen {
    int width = 0, height = 0, h_samp = 0, v_samp = 0;
    int check(int w, int h, int hs, int vs)
    {
        if (w == width && h == height && hs == h_samp && vs == v_samp) return HVQ_OK;
        { int rc = geometry_supported(w, h, hs, vs); if (rc) return rc; }
        width = w; height = h; h_samp = hs; v_samp = vs;
        return HVQ_OK;
    }
};

/* a picture in slot layout as the plane walk sees it: luma size and the chroma planes' shifts, of a stream or of a target */
struct SlotShape { int w, h, xs, ys; };
static inline SlotShape slot_shape(const Stream &s) { return { s.w, s.h, s.wshift, s.hshift }; }
static inline SlotShape slot_shape(int width, int height, int h_samp, int v_samp) { return { width, height, h_samp == 2, v_samp == 2 }; }

/* The three planes of one picture: `job(p, so, to, nx, ny, mx, my)` gets plane p's offset and size in a picture of shape `s` and in
 * one of shape `t`, and returns the plane's tiles, or a negative code, which ends the walk.  -> the picture's tiles, or that code.
 * Always inline: an entry point's loop over 65535 pictures calls nothing but what its job calls. */
template <class Job>
__attribute__((always_inline)) static inline int64_t plane_walk(const SlotShape &s, const SlotShape &t, Job job)
{
    size_t so = 0, to = 0;
    int64_t tiles = 0;
    for (int p = 0; p < 3; ++p) {
        const uint32_t nx = (uint32_t)(s.w >> (p ? s.xs : 0)), ny = (uint32_t)(s.h >> (p ? s.ys : 0));
        const uint32_t mx = (uint32_t)(t.w >> (p ? t.xs : 0)), my = (uint32_t)(t.h >> (p ? t.ys : 0));
        const int64_t r = job(p, so, to, nx, ny, mx, my);
        if (r < 0) return r;
        tiles += r;
        so += (size_t)nx * ny;
        to += (size_t)mx * my;
    }
    return tiles;
}

/* one shape on both sides: `job(p, off, nx, ny)` */
template <class Job>
__attribute__((always_inline)) static inline int64_t plane_walk(const SlotShape &s, Job job)
{
    return plane_walk(s, s, [&](int p, size_t off, size_t, uint32_t nx, uint32_t ny, uint32_t, uint32_t) { return job(p, off, nx, ny); });
}

/* a launch is a weak symbol: null where the kernel's file is not linked.  Refused before anything is allocated or enqueued */
template <class Launch>
static int kernel_check(Launch *launch, const char *kernel, const char *file, bool several = false)
{
    if (!launch) return fail(HVQ_E_NOGPU, "this build of the library has no %s kernel%s (%s is not linked)", kernel, several ? "s" : "", file);
    return HVQ_OK;
}

/* The tail: `count` pictures of at most `max_tiles` tiles (or workgroups) go to `launch` behind the upload of the table; a call whose
 * launch adds into its records has `zero_bytes` at `zero` cleared on the stream in front of it */
typedef hipError_t SlotLaunch(const void *tab_dev, int count, uint32_t max_tiles, hipStream_t stream);
static int table_enqueue(HvqContext *c, SlotLaunch *launch, const char *kernel, const char *file, const void *table, size_t bytes, int count,
                         uint32_t max_tiles, void *hip_stream, void *zero, size_t zero_bytes)
{
    { int rc = kernel_check(launch, kernel, file); if (rc) return rc; }
    return export_enqueue(c, table, bytes, hip_stream, [=](const void *t, hipStream_t st) {
        if (zero) { hipError_t e = hipMemsetAsync(zero, 0, zero_bytes, st); if (e != hipSuccess) return e; }
        return launch(t, count, max_tiles, st);
    });
}

/* ... of a table of jobs, or of bytes that a call has laid out itself */
template <class Job>
static int slot_enqueue(HvqContext *c, SlotLaunch *launch, const char *kernel, const char *file, const std::vector<Job> &table, int count,
                        uint32_t max_tiles, void *hip_stream, void *zero = nullptr, size_t zero_bytes = 0)
{
    static_assert(sizeof(Job) == 1 || sizeof(Job) % 16 == 0, "job tables are uploaded in 16-byte units");
    return table_enqueue(c, launch, kernel, file, table.data(), table.size() * sizeof(Job), count, max_tiles, hip_stream, zero, zero_bytes);
}

/* ---- The frame of the calls that read pictures and write records ("The record frame"): metrics, SSIM, checksums,
 * histograms, motion, JPEG, hashes.  The head is count_check (with GRID_ROW, hashes without) and record_out_check, the loop begins with
 * picture_source and picture_reference (above), the tail is slot_enqueue where one launch takes (table, count, most workgroups) ---- */

static const char GRID_ROW[] = " (one grid row each)";

/* the records of a call (`out`, `lengths`): the kernels store whole words of `align` bytes */
static int record_out_check(const char *name, const void *ptr, unsigned align)
{
    if (!ptr || ((uintptr_t)ptr & (align - 1u))) return fail(HVQ_E_ARG, "%s must be a non-null multiple of %u", name, align);
    return HVQ_OK;
}

/* Picture i (at `a`, of stream `sid`) for a job whose workgroups take `chunk` consecutive 16-byte units of ONE plane (metrics, checksums,
 * histograms): the planes, of ny, nc, nc bytes one behind the other, must be made of such units, `max_units` of them at the most where
 * the kernel counts them in fewer bits (0: no limit).  wg_first[0] is 0 already (the job was zeroed) -> the picture's workgroups, which
 * is wg_first[3], or a negative code.  Always inline, as plane_walk is. */
__attribute__((always_inline)) static inline int64_t unit_planes(const Stream &s, int i, int sid, const uint8_t *a, uint32_t chunk, uint32_t max_units,
                                                                 uint32_t plane_off[3], uint32_t units[3], uint32_t wg_first[4])
{
    const size_t ny = (size_t)s.w * s.h, nc = (size_t)(s.w >> s.wshift) * (size_t)(s.h >> s.hshift);
    if (((uintptr_t)a | ny | nc) & 15u) return fail(HVQ_E_ARG, "picture %d: a plane of stream %d is not made of 16-byte units", i, sid);
    if (max_units && ny / 16u > max_units) return fail(HVQ_E_ARG, "picture %d: a plane of stream %d has more than %u 16-byte units", i, sid, max_units);
    const size_t len[3] = { ny, nc, nc };
    size_t off = 0;
    for (int p = 0; p < 3; ++p) {
        plane_off[p] = (uint32_t)off;
        units[p] = (uint32_t)(len[p] / 16u);
        wg_first[p + 1] = wg_first[p] + (units[p] + chunk - 1u) / chunk;
        off += len[p];
    }
    return wg_first[3];
}

/* the hvq_*_force_* switches of the tests: -> the state before; `states` 3 where 2 is a state of its own (warp) */
template <class T>
static int force_switch(HvqContext *c, T HvqContext::*flag, int on, int states = 2)
{
    if (!c) return fail(HVQ_E_ARG, "bad arguments");
    const int was = (int)(c->*flag);
    c->*flag = (T)(states == 3 && on == 2 ? 2 : on != 0);
    return was;
}

HVQ_EXPORT int hvq_export_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, int format,
                                   const HvqExportDst *dst, void *hip_stream)
{
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    if (format != HVQ_FMT_RGB24 && format != HVQ_FMT_RGBP && format != HVQ_FMT_YUV444P) return fail(HVQ_E_ARG, "bad format %d", format);
    if (!n) return HVQ_OK;
    { int rc = chain_begin(c, n, streams, ordinals, nullptr, nullptr); if (rc) return rc; }
    std::vector<HvqRgbJob> jobs((size_t)n);
    int max_lanes = 0, wide = 1;
    for (int i = 0; i < n; ++i) {
        const uint8_t *src = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, nullptr, &src); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        const int64_t dense = format == HVQ_FMT_RGB24 ? (int64_t)s.w * 3 : (int64_t)s.w;
        const int64_t rp = dst[i].row_pitch ? dst[i].row_pitch : dense;
        const int64_t pp = format == HVQ_FMT_RGB24 ? 0 : dst[i].plane_pitch ? dst[i].plane_pitch : rp * s.h;
        if (!dst[i].ptr) return fail(HVQ_E_ARG, "null destination %d", i);
        if (rp < dense || rp > ((int64_t)1 << 40) || (format != HVQ_FMT_RGB24 && dst[i].plane_pitch > ((int64_t)1 << 48)))
            return fail(HVQ_E_ARG, "destination %d: row pitch %lld outside [%lld, 2^40] or plane pitch above 2^48", i, (long long)rp, (long long)dense);
        if (format != HVQ_FMT_RGB24 && pp < rp * s.h)
            return fail(HVQ_E_ARG, "destination %d: plane pitch %lld below row pitch x height %lld (planes overlap)", i, (long long)pp, (long long)(rp * s.h));
        if (((uintptr_t)dst[i].ptr | (uint64_t)rp | (uint64_t)pp) & 3u)
            return fail(HVQ_E_ARG, "destination %d: pointer, row pitch and plane pitch must be multiples of 4", i);
        const size_t ny = (size_t)s.w * s.h, nc = (size_t)(s.w >> s.wshift) * (size_t)(s.h >> s.hshift);
        jobs[(size_t)i] = HvqRgbJob{ src, src + ny, src + ny + nc, (uint8_t *)dst[i].ptr, rp, pp, s.w, s.h, s.wshift, s.hshift };
        if (s.w % 16) wide = 0;
        max_lanes = std::max(max_lanes, (s.w >> 2) * s.h);
    }
    return export_enqueue(c, jobs.data(), (size_t)n * sizeof(HvqRgbJob), hip_stream,
                          [=](const void *tab, hipStream_t st) { return hvq_launch_rgb(tab, n, max_lanes, wide, format, st); });
}

/* Picture metrics (include/hvqm4_amd.h: the specification): a third member of the export chain.  chain_begin over both sides of every
 * pair, picture_source and picture_reference per pair (zeros are a reference here); the memset of the records and the launch go behind
 * the job table on the caller's stream (export_enqueue). */
HVQ_EXPORT int hvq_picture_metrics(HvqContext *c, int n, const int *streams, const int *ordinals, const HvqMetricsRef *ref,
                                   uint64_t *out, void *hip_stream)
{
    if (!c || n < 0 || (n && (!streams || !ordinals))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures", GRID_ROW); if (rc) return rc; }
    if (!n) return HVQ_OK;
    { int rc = record_out_check("out", out, 8); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, nullptr, ref); if (rc) return rc; }
    std::vector<HvqMetricsJob> jobs((size_t)n);
    uint32_t max_wgs = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr, *b = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, nullptr, &a); if (rc) return rc; }
        { int rc = picture_reference(c, i, streams[i], ref ? ref + i : nullptr, nullptr, &b); if (rc) return rc; }
        HvqMetricsJob &j = jobs[(size_t)i];
        memset(&j, 0, sizeof j);
        const int64_t wgs = unit_planes(c->streams[(size_t)streams[i]], i, streams[i], a, HVQ_MT_CHUNK, 0, j.plane_off, j.units, j.wg_first);
        if (wgs < 0) return (int)wgs;
        j.a = (uint64_t)(uintptr_t)a; j.b = (uint64_t)(uintptr_t)b;
        j.out = (uint64_t)(uintptr_t)(out + (size_t)i * 12u);
        max_wgs = std::max(max_wgs, (uint32_t)wgs);
    }
    return slot_enqueue(c, hvq_launch_metrics, "metrics", "hvq_metrics.hip", jobs, n, max_wgs, hip_stream, out, (size_t)n * 96u);
}

/* Windows of SSIM per plane (include/hvqm4_amd.h): host only */
HVQ_EXPORT int hvq_ssim_windows(int width, int height, int h_samp, int v_samp, int32_t dims[3][2])
{
    { int rc = geometry_supported(width, height, h_samp, v_samp); if (rc) return rc; }
    const int cw = width >> (h_samp == 2), ch = height >> (v_samp == 2);
    const int w[3] = { width, cw, cw }, h[3] = { height, ch, ch };
    int total = 0;
    for (int k = 0; k < 3; ++k) {
        const int rows = std::max(h[k] / 4 - 1, 0), cols = std::max(w[k] / 4 - 1, 0);
        if (dims) { dims[k][0] = rows; dims[k][1] = cols; }
        total += rows * cols;
    }
    return total;
}

/* Windowed SSIM (include/hvqm4_amd.h: the specification): a fourth member of the export chain: chain_begin over both sides of every
 * pair, picture_source and picture_reference per pair, zeros refused here; the memset of the records and the launch go behind the job
 * table on the caller's stream (export_enqueue). */
HVQ_EXPORT int hvq_picture_ssim(HvqContext *c, int n, const int *streams, const int *ordinals, const HvqMetricsRef *ref,
                                int64_t *out, float *const *maps, void *hip_stream)
{
    if (!c || n < 0 || (n && (!streams || !ordinals))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures", GRID_ROW); if (rc) return rc; }
    if (!n) return HVQ_OK;
    { int rc = record_out_check("out", out, 8); if (rc) return rc; }
    if (!ref) return fail(HVQ_E_ARG, "SSIM needs a reference for every picture (ref is NULL)");
    for (int i = 0; maps && i < n; ++i)
        if ((uintptr_t)maps[i] & 3u) return fail(HVQ_E_ARG, "map %d: the pointer must be a multiple of 4", i);
    { int rc = chain_begin(c, n, streams, ordinals, nullptr, ref); if (rc) return rc; }
    std::vector<HvqSsimJob> jobs((size_t)n);
    uint32_t max_wgs = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr, *b = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, nullptr, &a); if (rc) return rc; }
        { int rc = picture_reference(c, i, streams[i], ref + i, "SSIM against a picture of zeros means nothing", &b); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        const uint32_t cw = (uint32_t)(s.w >> s.wshift), ch = (uint32_t)(s.h >> s.hshift);
        const uint32_t w[3] = { (uint32_t)s.w, cw, cw }, h[3] = { (uint32_t)s.h, ch, ch };
        if (((uintptr_t)a | w[0] | w[1] | h[0] | h[1]) & 3u) return fail(HVQ_E_ARG, "picture %d: a plane of stream %d is not made of 4 x 4 blocks", i, streams[i]);
        HvqSsimJob &j = jobs[(size_t)i];
        memset(&j, 0, sizeof j);
        j.a = (uint64_t)(uintptr_t)a; j.b = (uint64_t)(uintptr_t)b;
        j.out = (uint64_t)(uintptr_t)(out + (size_t)i * 6u);
        j.map = (uint64_t)(uintptr_t)(maps ? maps[i] : nullptr);
        uint32_t off = 0, moff = 0;
        for (int p = 0; p < 3; ++p) {
            j.plane_off[p] = off; j.map_off[p] = moff;
            j.bw[p] = w[p] / 4u; j.bh[p] = h[p] / 4u;
            const uint32_t rows = j.bh[p] ? j.bh[p] - 1u : 0u, cols = j.bw[p] ? j.bw[p] - 1u : 0u;
            const uint32_t tiles_y = rows && cols ? (rows + HVQ_SS_TR - 1u) / HVQ_SS_TR : 0u;
            j.tiles_x[p] = rows && cols ? (cols + HVQ_SS_TC - 1u) / HVQ_SS_TC : 1u;
            j.wg_first[p + 1] = j.wg_first[p] + tiles_y * j.tiles_x[p];
            off += w[p] * h[p]; moff += rows * cols;
        }
        max_wgs = std::max(max_wgs, j.wg_first[3]);
    }
    return slot_enqueue(c, hvq_launch_ssim, "SSIM", "hvq_ssim.hip", jobs, n, max_wgs, hip_stream, out, (size_t)n * 48u);
}

/* Checksums of resident pictures (include/hvqm4_amd.h: the specification): a fifth member of the export chain: chain_begin over the
 * resident pictures, picture_source with `src` per picture.  The memset of the accumulators and the two launches go behind the job
 * table on the caller's stream (export_enqueue); the accumulators are the context's own, reused by every call: the chain orders the
 * calls. */
HVQ_EXPORT int hvq_picture_checksums(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                     uint64_t *out, void *hip_stream)
{
    if (!c || n < 0 || (n && (!streams || !ordinals))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures", GRID_ROW); if (rc) return rc; }
    if (!n) return HVQ_OK;
    { int rc = record_out_check("out", out, 8); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqChecksumJob> jobs((size_t)n);
    uint32_t max_wgs = 0;
    size_t known_len[2] = { 0, 0 };                                /* x^(8 len) of the last two plane lengths seen: streams share geometries */
    uint32_t known_x[2] = { HVQ_CRC_ONE, HVQ_CRC_ONE };
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        HvqChecksumJob &j = jobs[(size_t)i];
        memset(&j, 0, sizeof j);
        const int64_t wgs = unit_planes(c->streams[(size_t)streams[i]], i, streams[i], a, HVQ_CK_CHUNK, HVQ_CK_MAX_UNITS, j.plane_off, j.units, j.wg_first);
        if (wgs < 0) return (int)wgs;
        j.a = (uint64_t)(uintptr_t)a;
        j.out = (uint64_t)(uintptr_t)(out + (size_t)i * 8u);
        for (int p = 0; p < 3; ++p) {
            const size_t len = (size_t)j.units[p] * 16u;
            const int slot = p != 0;
            if (known_len[slot] != len) { known_len[slot] = len; known_x[slot] = hvq_gf_xpow8(len); }
            j.xlen[p] = known_x[slot];
        }
        max_wgs = std::max(max_wgs, (uint32_t)wgs);
    }
    { int rc = kernel_check(hvq_launch_checksums, "checksum", "hvq_checksum.hip"); if (rc) return rc; }
    const size_t acc_bytes = (size_t)n * 96u;
    { int rc = scratch_grow(c, &c->ck_acc, &c->ck_cap, acc_bytes, 4096); if (rc) return rc; }
    uint8_t *acc = c->ck_acc;
    for (int i = 0; i < n; ++i) jobs[(size_t)i].acc = (uint64_t)(uintptr_t)(acc + (size_t)i * 96u);
    return slot_enqueue(c, hvq_launch_checksums, "checksum", "hvq_checksum.hip", jobs, n, max_wgs, hip_stream, acc, acc_bytes);
}

/* Histograms of resident pictures (include/hvqm4_amd.h: the specification): a sixth member of the export chain: chain_begin over the
 * resident pictures of both sides, picture_source with `src` and picture_reference per picture, zeros refused here.  The memset of the
 * records and the launch go behind the job table on the caller's stream (export_enqueue). */
HVQ_EXPORT int hvq_picture_histograms(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src, int mode,
                                      const HvqMetricsRef *ref, uint32_t *out, void *hip_stream)
{
    static_assert(HVQ_HIST_BINS == HVQ_HG_BINS, "the kernel's bins are the header's");
    if (!c || n < 0 || (n && (!streams || !ordinals))) return fail(HVQ_E_ARG, "bad arguments");
    if (mode != HVQ_HIST_VALUES && mode != HVQ_HIST_ABSDIFF) return fail(HVQ_E_ARG, "bad mode %d", mode);
    if (mode == HVQ_HIST_VALUES && ref) return fail(HVQ_E_ARG, "HVQ_HIST_VALUES takes no reference (ref must be NULL)");
    { int rc = count_check(n, "pictures", GRID_ROW); if (rc) return rc; }
    if (!n) return HVQ_OK;
    { int rc = record_out_check("out", out, 4); if (rc) return rc; }
    if (mode == HVQ_HIST_ABSDIFF && !ref) return fail(HVQ_E_ARG, "HVQ_HIST_ABSDIFF needs a reference for every picture (ref is NULL)");
    { int rc = chain_begin(c, n, streams, ordinals, src, ref); if (rc) return rc; }
    std::vector<HvqHistogramJob> jobs((size_t)n);
    uint32_t max_wgs = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr, *b = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        /* no reference (HVQ_HIST_VALUES) is none to refuse; a given one of zeros is */
        { int rc = picture_reference(c, i, streams[i], ref ? ref + i : nullptr, "|a - 0| is a itself, HVQ_HIST_VALUES gives it", &b); if (rc) return rc; }
        HvqHistogramJob &j = jobs[(size_t)i];
        memset(&j, 0, sizeof j);
        const int64_t wgs = unit_planes(c->streams[(size_t)streams[i]], i, streams[i], a, HVQ_HG_CHUNK, HVQ_HG_MAX_UNITS, j.plane_off, j.units, j.wg_first);
        if (wgs < 0) return (int)wgs;
        j.a = (uint64_t)(uintptr_t)a; j.b = (uint64_t)(uintptr_t)b;
        j.out = (uint64_t)(uintptr_t)(out + (size_t)i * 3u * HVQ_HIST_BINS);
        max_wgs = std::max(max_wgs, (uint32_t)wgs);
    }
    return slot_enqueue(c, hvq_launch_histograms, "histogram", "hvq_histogram.hip", jobs, n, max_wgs, hip_stream, out, (size_t)n * 3u * HVQ_HIST_BINS * sizeof(uint32_t));
}

/* Blocks of a motion field (include/hvqm4_amd.h): host only */
HVQ_EXPORT int hvq_motion_blocks(int width, int height, int h_samp, int v_samp, int block, int32_t dims[2])
{
    { int rc = geometry_supported(width, height, h_samp, v_samp); if (rc) return rc; }
    if (block != 8 && block != 16) return fail(HVQ_E_ARG, "block %d (8 or 16)", block);
    if (width % block || height % block) return fail(HVQ_E_ARG, "blocks of %d do not tile a %d x %d picture", block, width, height);
    if (dims) { dims[0] = height / block; dims[1] = width / block; }
    return (height / block) * (width / block);
}

/* Motion fields between resident pictures (include/hvqm4_amd.h: the specification): a seventh member of the export chain: chain_begin
 * over both sides of every pair, picture_source and picture_reference per pair, zeros refused here.  Only the launch goes behind the
 * job table on the caller's stream (export_enqueue): it writes every record, nothing is zeroed in front of it. */
HVQ_EXPORT int hvq_picture_motion(HvqContext *c, int n, const int *streams, const int *ordinals, const HvqMetricsRef *ref,
                                  int block, int radius, int32_t *const *out, void *hip_stream)
{
    static_assert(HVQ_MOTION_MAX_RADIUS == HVQ_MV_MAX_RADIUS, "the kernel's largest radius is the header's");
    if (!c || n < 0 || (n && (!streams || !ordinals))) return fail(HVQ_E_ARG, "bad arguments");
    if (block != 8 && block != 16) return fail(HVQ_E_ARG, "block %d (8 or 16)", block);
    if (radius < 0 || radius > HVQ_MOTION_MAX_RADIUS) return fail(HVQ_E_ARG, "radius %d outside [0, %d]", radius, HVQ_MOTION_MAX_RADIUS);
    { int rc = count_check(n, "pictures", GRID_ROW); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (!out) return fail(HVQ_E_ARG, "out is NULL");
    if (!ref) return fail(HVQ_E_ARG, "motion needs a reference for every picture (ref is NULL)");
    for (int i = 0; i < n; ++i) { int rc = slot_pointer_check("field", i, out[i]); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, nullptr, ref); if (rc) return rc; }
    std::vector<HvqMotionJob> jobs((size_t)n);
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr, *b = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, nullptr, &a); if (rc) return rc; }
        { int rc = picture_reference(c, i, streams[i], ref + i, "motion against a picture of zeros means nothing", &b); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        if (s.w % block || s.h % block) return fail(HVQ_E_ARG, "picture %d: blocks of %d do not tile stream %d (%d x %d)", i, block, streams[i], s.w, s.h);
        if ((uintptr_t)a & 15u || s.w >= (int)HVQ_MV_MAX_SIDE || s.h >= (int)HVQ_MV_MAX_SIDE)
            return fail(HVQ_E_ARG, "picture %d: stream %d (%d x %d) is beyond what the motion kernel addresses", i, streams[i], s.w, s.h);
        HvqMotionJob &j = jobs[(size_t)i];
        memset(&j, 0, sizeof j);
        j.a = (uint64_t)(uintptr_t)a; j.b = (uint64_t)(uintptr_t)b;
        j.out = (uint64_t)(uintptr_t)out[i];
        j.w = (uint32_t)s.w; j.h = (uint32_t)s.h;
        j.rows = j.h / (uint32_t)block; j.cols = j.w / (uint32_t)block;
        j.tiles_x = (j.w + HVQ_MV_TILE - 1u) / HVQ_MV_TILE;
        j.tiles = j.tiles_x * ((j.h + HVQ_MV_TILE - 1u) / HVQ_MV_TILE);
        max_tiles = std::max(max_tiles, j.tiles);
    }
    { int rc = kernel_check(hvq_launch_motion, "motion", "hvq_motion.hip"); if (rc) return rc; }
    return export_enqueue(c, jobs.data(), (size_t)n * sizeof(HvqMotionJob), hip_stream,
                          [=](const void *tab, hipStream_t st) { return hvq_launch_motion(tab, n, max_tiles, block, radius, st); });
}

/* The header and the bound of a JPEG file (include/hvqm4_amd.h): host only */
static int jpeg_geometry(int width, int height, int h_samp, int v_samp)
{
    { int rc = geometry_supported(width, height, h_samp, v_samp); if (rc) return rc; }
    if (width >= (int)HVQ_JP_MAX_SIDE || height >= (int)HVQ_JP_MAX_SIDE || hvq_jpeg_bound_of((uint32_t)width, (uint32_t)height, (uint32_t)h_samp, (uint32_t)v_samp) >> 32)
        return fail(HVQ_E_GEOMETRY, "%d x %d is beyond what a JPEG file of this library holds", width, height);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_jpeg_header(int width, int height, int h_samp, int v_samp, int quality, uint8_t *dst, size_t cap, size_t *len)
{
    { int rc = jpeg_geometry(width, height, h_samp, v_samp); if (rc) return rc; }
    if (quality < 1 || quality > 100) return fail(HVQ_E_ARG, "quality %d outside [1, 100]", quality);
    if (len) *len = HVQ_JPEG_HEADER_BYTES;
    if (!dst || cap < HVQ_JPEG_HEADER_BYTES) return fail(HVQ_E_ARG, "the header takes %u bytes", HVQ_JPEG_HEADER_BYTES);
    uint8_t buf[HVQ_JPEG_HEADER_SLOT];
    if (hvq_jpeg_write_header((uint32_t)width, (uint32_t)height, (uint32_t)h_samp, (uint32_t)v_samp, quality, buf) != HVQ_JPEG_HEADER_BYTES)
        return fail(HVQ_E_ARG, "internal: the header is not %u bytes", HVQ_JPEG_HEADER_BYTES);
    memcpy(dst, buf, HVQ_JPEG_HEADER_BYTES);
    return HVQ_OK;
}

HVQ_EXPORT size_t hvq_jpeg_bound(int width, int height, int h_samp, int v_samp)
{
    if (jpeg_geometry(width, height, h_samp, v_samp)) return 0;
    return (size_t)hvq_jpeg_bound_of((uint32_t)width, (uint32_t)height, (uint32_t)h_samp, (uint32_t)v_samp);
}

/* Baseline JPEG files of resident pictures (include/hvqm4_amd.h: the specification): an eighth member of the export chain: chain_begin
 * over the resident pictures, picture_source with `src` per picture.  The three launches go behind the job table on the caller's
 * stream (export_enqueue); the table carries the call's quantisers and one header per distinct geometry behind the jobs; the scratch
 * is the context's own, reused by every call: the chain orders the calls. */
HVQ_EXPORT int hvq_encode_jpeg(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src, int quality,
                               void *const *out, const uint64_t *cap, uint64_t *lengths, void *hip_stream)
{
    static_assert(HVQ_JPEG_HEADER == HVQ_JPEG_HEADER_BYTES, "the kernel's header length is the header's");
    if (!c || n < 0 || (n && (!streams || !ordinals))) return fail(HVQ_E_ARG, "bad arguments");
    if (quality < 1 || quality > 100) return fail(HVQ_E_ARG, "quality %d outside [1, 100]", quality);
    { int rc = count_check(n, "pictures", GRID_ROW); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (!out || !cap) return fail(HVQ_E_ARG, "out or cap is NULL");
    { int rc = record_out_check("lengths", lengths, 8); if (rc) return rc; }
    for (int i = 0; i < n; ++i) {
        { int rc = slot_pointer_check("file", i, out[i]); if (rc) return rc; }
        if (cap[i] < HVQ_JPEG_HEADER_BYTES + 2u) return fail(HVQ_E_ARG, "file %d: %llu bytes hold not even the header and EOI (%u)", i, (unsigned long long)cap[i], HVQ_JPEG_HEADER_BYTES + 2u);
    }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    const size_t quant_off = (size_t)n * sizeof(HvqJpegJob), hdr0 = quant_off + sizeof(HvqJpegQuant);
    std::vector<uint8_t> table(hdr0);
    std::vector<uint32_t> geoms;                                        /* w, h, hs << 4 | vs of every header in the table */
    uint32_t max_mh = 0;
    size_t scr_dwords = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        const uint32_t hs = 1u << s.wshift, vs = 1u << s.hshift;
        if (((uintptr_t)a & 15u) || s.w % 8 || s.h % 8 || s.w >= (int)HVQ_JP_MAX_SIDE || s.h >= (int)HVQ_JP_MAX_SIDE || hs > 2u || vs > 2u ||
            hvq_jpeg_bound_of((uint32_t)s.w, (uint32_t)s.h, hs, vs) >> 32)
            return fail(HVQ_E_ARG, "picture %d: stream %d (%d x %d) is beyond what the JPEG kernels address", i, streams[i], s.w, s.h);
        HvqJpegJob j;
        memset(&j, 0, sizeof j);
        j.src = (uint64_t)(uintptr_t)a; j.out = (uint64_t)(uintptr_t)out[i]; j.cap = cap[i]; j.len = (uint64_t)(uintptr_t)(lengths + i);
        j.w = (uint32_t)s.w; j.h = (uint32_t)s.h; j.hs = hs; j.vs = vs;
        j.mw = hvq_jpeg_mw(j.w, hs); j.mh = hvq_jpeg_mh(j.h, vs);
        j.scr_first = (uint32_t)scr_dwords;
        scr_dwords += (size_t)j.mh + 1u;
        if (scr_dwords >> 31) return fail(HVQ_E_ARG, "%d pictures have more restart intervals than one call takes", n);
        max_mh = std::max(max_mh, j.mh);
        size_t g = 0;
        while (g < geoms.size() && !(geoms[g] == j.w && geoms[g + 1] == j.h && geoms[g + 2] == (hs << 4 | vs))) g += 3;
        if (g == geoms.size()) {
            geoms.insert(geoms.end(), { j.w, j.h, hs << 4 | vs });
            table.resize(table.size() + HVQ_JPEG_HEADER_SLOT);
            hvq_jpeg_write_header(j.w, j.h, hs, vs, quality, table.data() + table.size() - HVQ_JPEG_HEADER_SLOT);
        }
        j.hdr_off = (uint32_t)(hdr0 + g / 3u * HVQ_JPEG_HEADER_SLOT);
        memcpy(table.data() + (size_t)i * sizeof j, &j, sizeof j);
    }
    HvqJpegQuant qt;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) qt.q[t][k] = hvq_jpeg_qpack(hvq_jpeg_q(HVQ_JPEG_QBASE[t][k], quality));
    memcpy(table.data() + quant_off, &qt, sizeof qt);
    { int rc = kernel_check(hvq_launch_jpeg, "JPEG", "hvq_jpeg.hip", true); if (rc) return rc; }
    { int rc = scratch_grow(c, &c->jp_scr, &c->jp_cap, scr_dwords, 1024); if (rc) return rc; }
    uint32_t *scr = c->jp_scr;
    return export_enqueue(c, table.data(), table.size(), hip_stream,
                          [=](const void *tab, hipStream_t st) { return hvq_launch_jpeg(tab, n, max_mh, (uint32_t)quant_off, scr, st); });
}

/* Perceptual hashes of resident pictures (include/hvqm4_amd.h: the specification): a ninth member of the export chain: chain_begin
 * over the resident pictures, picture_source with `src` per picture.  The memset of the cells and the two launches go behind the job
 * table on the caller's stream (export_enqueue), HVQ_PH_BATCH pictures a launch pair: the cells are the context's own, reused by every
 * pair and every call -- the stream orders the pairs, the chain the calls. */
#ifndef HVQ_PH_CPW
#define HVQ_PH_CPW HVQ_PH_MAX_CPW      /* most row cells of a workgroup (measurements: 1, 2, 4) */
#endif
HVQ_EXPORT int hvq_picture_hashes(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                  uint64_t *out, void *hip_stream)
{
    if (!c || n < 0 || (n && (!streams || !ordinals))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    { int rc = record_out_check("out", out, 8); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqHashJob> jobs((size_t)n);
    uint32_t max_wgs = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        if (((uintptr_t)a & 15u) || (s.w & 7) || (s.h & 7) || s.w < 8 || s.h < 8 || s.w > (int)HVQ_PH_MAX_SIDE || s.h > (int)HVQ_PH_MAX_SIDE)
            return fail(HVQ_E_ARG, "picture %d: stream %d (%d x %d) is beyond what the hash kernels address", i, streams[i], s.w, s.h);
        HvqHashJob &j = jobs[(size_t)i];
        memset(&j, 0, sizeof j);
        j.a = (uint64_t)(uintptr_t)a;
        j.out = (uint64_t)(uintptr_t)(out + (size_t)i * 4u);
        j.w = (uint32_t)s.w; j.h = (uint32_t)s.h;
        j.units = j.w / ((j.w & 8u) ? 8u : 16u);
        j.lanes_x = std::min(j.units, HVQ_PH_LANES);
        /* as many row cells a workgroup as leave every cell a whole row of lanes: the work a lane does once per row cell (the column
         * weights) is then shared by more rows (1, 2, 4 and 8 were measured) */
        j.cells_pw = 1; j.sub_shift = 8;
        while (j.cells_pw < HVQ_PH_CPW && (HVQ_PH_LANES >> 1 >> (8u - j.sub_shift)) >= j.lanes_x) { j.cells_pw *= 2u; --j.sub_shift; }
        j.rows_pp = (HVQ_PH_LANES / j.cells_pw) / j.lanes_x;
        j.wgs = HVQ_PH_ROWS / j.cells_pw * ((j.units + HVQ_PH_LANES - 1u) / HVQ_PH_LANES);
        max_wgs = std::max(max_wgs, j.wgs);
    }
    { int rc = kernel_check(hvq_launch_hashes, "hash", "hvq_phash.hip", true); if (rc) return rc; }
    const size_t cell_bytes = (size_t)HVQ_PH_CELLS * 8u;
    const size_t acc_bytes = (size_t)std::min(n, (int)HVQ_PH_BATCH) * cell_bytes;
    { int rc = scratch_grow(c, &c->ph_acc, &c->ph_cap, acc_bytes, 4096, align_up((size_t)HVQ_PH_BATCH * cell_bytes, 4096)); if (rc) return rc; }
    uint8_t *acc = c->ph_acc;
    for (int i = 0; i < n; ++i) jobs[(size_t)i].acc = (uint64_t)(uintptr_t)(acc + (size_t)(i % (int)HVQ_PH_BATCH) * cell_bytes);
    return export_enqueue(c, jobs.data(), (size_t)n * sizeof(HvqHashJob), hip_stream,
                          [=](const void *tab, hipStream_t st) {
                              for (int at = 0; at < n; at += (int)HVQ_PH_BATCH) {
                                  const int cnt = std::min(n - at, (int)HVQ_PH_BATCH);
                                  hipError_t e = hipMemsetAsync(acc, 0, (size_t)cnt * cell_bytes, st);    /* the first launch adds into them */
                                  if (e == hipSuccess) e = hvq_launch_hashes((const HvqHashJob *)tab + at, cnt, max_wgs, st);
                                  if (e != hipSuccess) return e;
                              }
                              return hipSuccess;
                          });
}

/* Nearest hashes (include/hvqm4_amd.h: the specification).  The call reads no resident picture: no member of the export chain, one launch
 * on the caller's stream. */
HVQ_EXPORT int hvq_hash_nearest(HvqContext *c, const uint64_t *q, int nq, int q_stride, const uint64_t *db, int ndb, int db_stride,
                                int64_t self_offset, int threshold, int32_t *out, void *hip_stream)
{
    static_assert(HVQ_HASH_NEAREST_MAX == HVQ_HN_MAX, "the kernel's key holds the header's counts");
    if (!c) return fail(HVQ_E_ARG, "bad arguments");
    if (nq < 0 || nq > HVQ_HASH_NEAREST_MAX || ndb < 0 || ndb > HVQ_HASH_NEAREST_MAX)
        return fail(HVQ_E_ARG, "%d queries against %d hashes: each count lies in [0, %d]", nq, ndb, HVQ_HASH_NEAREST_MAX);
    if (q_stride < 1 || db_stride < 1) return fail(HVQ_E_ARG, "strides %d and %d: a stride counts 64-bit words and is at least 1", q_stride, db_stride);
    if (threshold < 0 || threshold > 64) return fail(HVQ_E_ARG, "threshold %d outside [0, 64]", threshold);
    if (!nq) return HVQ_OK;
    if (!q || ((uintptr_t)q & 7u)) return fail(HVQ_E_ARG, "q must be a non-null multiple of 8");
    if (ndb && (!db || ((uintptr_t)db & 7u))) return fail(HVQ_E_ARG, "db must be a non-null multiple of 8");
    if (!out || ((uintptr_t)out & 15u)) return fail(HVQ_E_ARG, "out must be a non-null multiple of 16");
    { int rc = kernel_check(hvq_launch_hash_nearest, "hash", "hvq_phash.hip", true); if (rc) return rc; }
    HIPCHK(hipSetDevice(c->device));
    /* an offset that admits every candidate for every query is "all" */
    const int64_t off = self_offset < 0 || self_offset >= (int64_t)ndb ? -1 : self_offset;
    HIPCHK(hvq_launch_hash_nearest(q, (uint32_t)nq, (uint32_t)q_stride, db, (uint32_t)ndb, (uint32_t)db_stride, off, (uint32_t)threshold, out,
                                   (hipStream_t)hip_stream));
    return HVQ_OK;
}

/* Scaled copies of resident pictures in slot layout (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "The slot-layout frame") */
HVQ_EXPORT int64_t hvq_scale_bytes(int width, int height, int h_samp, int v_samp)
{
    { int rc = geometry_supported(width, height, h_samp, v_samp); if (rc) return rc; }
    return (int64_t)width * height + 2 * (int64_t)(width >> (h_samp == 2)) * (height >> (v_samp == 2));
}

HVQ_EXPORT int hvq_scale_body(int nx, int ny, int mx, int my)
{
    if (nx < 1 || ny < 1 || mx < 1 || my < 1 || nx > 8192 || ny > 8192 || mx > 8192 || my > 8192)
        return fail(HVQ_E_ARG, "%d x %d -> %d x %d: a plane has 1 .. 8192 samples a side", nx, ny, mx, my);
    if (nx > (int)HVQ_SC_MAX_RATIO * mx || ny > (int)HVQ_SC_MAX_RATIO * my)
        return fail(HVQ_E_ARG, "%d x %d -> %d x %d: a reduction beyond %u is refused", nx, ny, mx, my, HVQ_SC_MAX_RATIO);
    return (int)hvq_sc_body((uint32_t)nx, (uint32_t)ny, (uint32_t)mx, (uint32_t)my);
}

HVQ_EXPORT int hvq_scale_force_direct(HvqContext *c, int on) { return force_switch(c, &HvqContext::sc_force_direct, on); }

HVQ_EXPORT int hvq_scale_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                  const HvqScaleDst *dst, void *hip_stream)
{
    static_assert(HVQ_SCALE_DIRECT == (int)HVQ_SC_DIRECT && HVQ_SCALE_TILED == (int)HVQ_SC_TILED && HVQ_SCALE_MAX_RATIO == (int)HVQ_SC_MAX_RATIO,
                  "the header's names are the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqScaleJob> jobs((size_t)n * 3u);
    uint32_t max_tiles = 0;
    /* a call usually repeats few shapes: the geometry check and the multipliers of a plane are kept from the picture before */
    TargetSeen seen;
    HvqScaleJob last[3];
    memset(last, 0, sizeof last);
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        const HvqScaleDst &d = dst[i];
        { int rc = slot_pointer_check("destination", i, d.ptr); if (rc) return rc; }
        { int rc = seen.check(d.width, d.height, d.h_samp, d.v_samp); if (rc) return rc; }
        int cx = d.crop_x, cy = d.crop_y, cw = d.crop_w, ch = d.crop_h;
        if (cw == 0) {
            if (cx || cy || ch) return fail(HVQ_E_ARG, "destination %d: crop_w == 0 means the whole picture and takes the other three as 0", i);
            cw = s.w; ch = s.h;
        }
        if (cx < 0 || cy < 0 || cw <= 0 || ch <= 0 || cx > s.w - cw || cy > s.h - ch)
            return fail(HVQ_E_ARG, "destination %d: the crop %d, %d, %d x %d is empty or leaves the %d x %d picture", i, cx, cy, cw, ch, s.w, s.h);
        if (((cx | cw) & ((1 << s.wshift) - 1)) || ((cy | ch) & ((1 << s.hshift) - 1)))
            return fail(HVQ_E_ARG, "destination %d: the crop %d, %d, %d x %d does not lie on the chroma samples of stream %d", i, cx, cy, cw, ch, streams[i]);
        if (cw < 8 || ch < 8) return fail(HVQ_E_ARG, "destination %d: a cropped source of %d x %d is below 8 x 8", i, cw, ch);
        const int64_t tiles = plane_walk(slot_shape(s), slot_shape(d.width, d.height, d.h_samp, d.v_samp),
                                         [&](int p, size_t so, size_t to, uint32_t pitch, uint32_t, uint32_t mx, uint32_t my) -> int64_t {
            const int xs = p ? s.wshift : 0, ys = p ? s.hshift : 0;
            const uint32_t nx = (uint32_t)(cw >> xs), ny = (uint32_t)(ch >> ys);
            if (nx > HVQ_SC_MAX_RATIO * mx || ny > HVQ_SC_MAX_RATIO * my)
                return fail(HVQ_E_ARG, "destination %d, plane %d: %u x %u -> %u x %u is a reduction beyond %u", i, p, nx, ny, mx, my, HVQ_SC_MAX_RATIO);
            HvqScaleJob &j = jobs[(size_t)i * 3u + (size_t)p];
            const uint64_t from = (uint64_t)(uintptr_t)(a + so + (size_t)(cy >> ys) * pitch + (size_t)(cx >> xs));
            const uint64_t to_ptr = (uint64_t)(uintptr_t)((uint8_t *)d.ptr + to);
            HvqScaleJob &l = last[p];
            if (l.nx == nx && l.ny == ny && l.mx == mx && l.my == my && ((l.body & HVQ_SC_TILED) == 0) == (c->sc_force_direct || hvq_sc_body(nx, ny, mx, my) == HVQ_SC_DIRECT)) {
                j = l;
                j.src = from; j.dst = to_ptr; j.pitch = pitch;
            } else {
                j = l = hvq_sc_job(from, pitch, nx, ny, to_ptr, mx, my, c->sc_force_direct);
            }
            return j.tiles;
        });
        if (tiles < 0) return (int)tiles;
        max_tiles = std::max(max_tiles, (uint32_t)tiles);
    }
    return slot_enqueue(c, hvq_launch_scale, "scale", "hvq_scale.hip", jobs, n, max_tiles, hip_stream);
}

/* Filtered copies of resident pictures in slot layout (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "The slot-layout frame"):
 * behind the jobs goes the table of the planes' filters with the taps widened to dwords */
static int filter_plane_check(const HvqPlaneFilter &p, const char *plane)
{
    if (p.terms != 1 && p.terms != 2) return fail(HVQ_E_ARG, "%s filter: %d terms (1 or 2)", plane, p.terms);
    if (p.combine != HVQ_FLT_SUM && p.combine != HVQ_FLT_ABS_SUM && p.combine != HVQ_FLT_SUM_ABS) return fail(HVQ_E_ARG, "%s filter: combine %d", plane, p.combine);
    if (p.shift < 0 || p.shift > HVQ_FLT_MAX_SHIFT) return fail(HVQ_E_ARG, "%s filter: shift %d outside 0 .. %d", plane, p.shift, HVQ_FLT_MAX_SHIFT);
    if (p.bias < -255 || p.bias > 255) return fail(HVQ_E_ARG, "%s filter: bias %d outside -255 .. 255", plane, p.bias);
    int64_t gain = 0;
    for (int t = 0; t < p.terms; ++t) {
        const HvqFilterTerm &T = p.term[t];
        if (T.rx < 0 || T.rx > HVQ_FLT_MAX_RADIUS || T.ry < 0 || T.ry > HVQ_FLT_MAX_RADIUS)
            return fail(HVQ_E_ARG, "%s filter, term %d: radii %d, %d outside 0 .. %d", plane, t, T.rx, T.ry, HVQ_FLT_MAX_RADIUS);
        int64_t ax = 0, ay = 0;
        for (int i = 0; i < HVQ_FLT_MAX_TAPS; ++i) {
            if (i > 2 * T.rx && T.wx[i]) return fail(HVQ_E_ARG, "%s filter, term %d: wx[%d] = %d lies beyond the %d taps of radius %d", plane, t, i, T.wx[i], 2 * T.rx + 1, T.rx);
            if (i > 2 * T.ry && T.wy[i]) return fail(HVQ_E_ARG, "%s filter, term %d: wy[%d] = %d lies beyond the %d taps of radius %d", plane, t, i, T.wy[i], 2 * T.ry + 1, T.ry);
            ax += T.wx[i] < 0 ? -(int64_t)T.wx[i] : T.wx[i];
            ay += T.wy[i] < 0 ? -(int64_t)T.wy[i] : T.wy[i];
        }
        gain += ax * ay;
    }
    if (gain < 1 || gain > HVQ_FLT_MAX_GAIN) return fail(HVQ_E_ARG, "%s filter: a gain of %lld (1 .. %d)", plane, (long long)gain, HVQ_FLT_MAX_GAIN);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_filter_check(const HvqFilter *f)
{
    if (!f) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = filter_plane_check(f->luma, "luma"); if (rc) return rc; }
    return filter_plane_check(f->chroma, "chroma");
}

/* a checked plane filter as the kernel reads it */
static HvqFilterPlaneDev filter_plane_dev(const HvqPlaneFilter &p)
{
    HvqFilterPlaneDev d;
    memset(&d, 0, sizeof d);
    d.terms = p.terms; d.combine = p.combine; d.shift = p.shift; d.bias = p.bias;
    d.half = p.shift ? 1 << (p.shift - 1) : 0;
    for (int t = 0; t < p.terms; ++t) {
        d.term[t].rx = p.term[t].rx; d.term[t].ry = p.term[t].ry;
        d.rmax = std::max(d.rmax, p.term[t].ry);
        for (int i = 0; i < HVQ_FLT_MAX_TAPS; ++i) { d.term[t].wx[i] = p.term[t].wx[i]; d.term[t].wy[i] = p.term[t].wy[i]; }
    }
    return d;
}

HVQ_EXPORT int hvq_filter_force_filter(HvqContext *c, int on) { return force_switch(c, &HvqContext::fl_force_filter, on); }

HVQ_EXPORT int hvq_filter_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                   const HvqFilter *filters, int nfilters, const int *which, void *const *dst, void *hip_stream)
{
    static_assert(HVQ_FLT_MAX_RADIUS == (int)HVQ_FL_MAX_R && HVQ_FLT_MAX_TAPS == 2 * HVQ_FLT_MAX_RADIUS + 1 && HVQ_FLT_MAX_TAPS <= 32,
                  "the header's limits are the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst || !filters))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nfilters < 1 || nfilters > HVQ_FLT_MAX_FILTERS) return fail(HVQ_E_ARG, "%d filters: one call takes 1 .. %d", nfilters, HVQ_FLT_MAX_FILTERS);
    for (int f = 0; f < nfilters; ++f) { int rc = hvq_filter_check(filters + f); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    const size_t job_bytes = (size_t)n * 3u * sizeof(HvqFilterJob), tab_bytes = (size_t)nfilters * 2u * sizeof(HvqFilterPlaneDev);
    std::vector<uint8_t> up(job_bytes + tab_bytes);
    HvqFilterJob *jobs = (HvqFilterJob *)up.data();
    HvqFilterPlaneDev *tab = (HvqFilterPlaneDev *)(up.data() + job_bytes);
    std::vector<int> copy((size_t)nfilters * 2u);
    for (int f = 0; f < nfilters; ++f) {
        tab[2 * f] = filter_plane_dev(filters[f].luma);
        tab[2 * f + 1] = filter_plane_dev(filters[f].chroma);
        for (int p = 0; p < 2; ++p) copy[(size_t)(2 * f + p)] = !c->fl_force_filter && hvq_fl_is_identity(&tab[2 * f + p]);
    }
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("destination", i, dst[i]); if (rc) return rc; }
        const int f = which ? which[i] : 0;
        if (f < 0 || f >= nfilters) return fail(HVQ_E_ARG, "picture %d: filter %d of %d", i, f, nfilters);
        uint8_t *const b = (uint8_t *)dst[i];
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            const uint32_t pf = (uint32_t)(2 * f + (p ? 1 : 0));
            HvqFilterJob &j = jobs[(size_t)i * 3u + (size_t)p];
            j = hvq_fl_job((uint64_t)(uintptr_t)(a + off), (uint64_t)(uintptr_t)(b + off), nx, ny, pf, copy[pf]);
            return j.tiles;
        }));
    }
    return slot_enqueue(c, hvq_launch_filter, "filter", "hvq_filter.hip", up, n, max_tiles, hip_stream);
}

/* Rank filters on resident pictures in slot layout (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "The slot-layout frame") */
static int rank_plane_check(const HvqRankPlane &p, const char *plane)
{
    if (p.op != HVQ_RNK_MIN && p.op != HVQ_RNK_MAX && p.op != HVQ_RNK_RANGE && p.op != HVQ_RNK_MEDIAN) return fail(HVQ_E_ARG, "%s rank: op %d", plane, p.op);
    if (p.rx < 0 || p.rx > HVQ_RNK_MAX_RADIUS || p.ry < 0 || p.ry > HVQ_RNK_MAX_RADIUS)
        return fail(HVQ_E_ARG, "%s rank: radii %d, %d outside 0 .. %d", plane, p.rx, p.ry, HVQ_RNK_MAX_RADIUS);
    if (p.op == HVQ_RNK_MEDIAN && (p.rx != p.ry || p.rx > 2)) return fail(HVQ_E_ARG, "%s rank: a median of radii %d, %d (1 x 1, 3 x 3 or 5 x 5)", plane, p.rx, p.ry);
    if (p.pad) return fail(HVQ_E_ARG, "%s rank: pad %d (0)", plane, p.pad);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_rank_check(const HvqRank *r)
{
    if (!r) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = rank_plane_check(r->luma, "luma"); if (rc) return rc; }
    return rank_plane_check(r->chroma, "chroma");
}

HVQ_EXPORT int hvq_rank_force_general(HvqContext *c, int on) { return force_switch(c, &HvqContext::rk_force_general, on); }

HVQ_EXPORT int hvq_rank_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                 const HvqRank *ranks, int nranks, const int *which, void *const *dst, void *hip_stream)
{
    static_assert(HVQ_RNK_MAX_RADIUS == (int)HVQ_RK_MAX_R && HVQ_RNK_MIN == (int)HVQ_RK_OP_MIN && HVQ_RNK_MAX == (int)HVQ_RK_OP_MAX &&
                  HVQ_RNK_RANGE == (int)HVQ_RK_OP_RANGE && HVQ_RNK_MEDIAN == (int)HVQ_RK_OP_MEDIAN, "the header's values are the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst || !ranks))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nranks < 1 || nranks > HVQ_RNK_MAX_RANKS) return fail(HVQ_E_ARG, "%d ranks: one call takes 1 .. %d", nranks, HVQ_RNK_MAX_RANKS);
    for (int r = 0; r < nranks; ++r) { int rc = hvq_rank_check(ranks + r); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqRankJob> jobs((size_t)n * 3u);
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("destination", i, dst[i]); if (rc) return rc; }
        const int r = which ? which[i] : 0;
        if (r < 0 || r >= nranks) return fail(HVQ_E_ARG, "picture %d: rank %d of %d", i, r, nranks);
        uint8_t *const b = (uint8_t *)dst[i];
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            const HvqRankPlane &rp = p ? ranks[r].chroma : ranks[r].luma;
            HvqRankJob &j = jobs[(size_t)i * 3u + (size_t)p];
            j = hvq_rk_job((uint64_t)(uintptr_t)(a + off), (uint64_t)(uintptr_t)(b + off), nx, ny, (uint32_t)rp.op, (uint32_t)rp.rx, (uint32_t)rp.ry, c->rk_force_general);
            return j.tiles;
        }));
    }
    return slot_enqueue(c, hvq_launch_rank, "rank", "hvq_rank.hip", jobs, n, max_tiles, hip_stream);
}

/* Bilateral filters on resident pictures in slot layout (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "The slot-layout frame"):
 * the call's parameter sets go behind the jobs in the same upload, as they stand in the header */
static int bilateral_plane_check(const HvqBilateralPlane &p, const char *plane)
{
    if (p.rx < 0 || p.rx > HVQ_BIL_MAX_RADIUS || p.ry < 0 || p.ry > HVQ_BIL_MAX_RADIUS)
        return fail(HVQ_E_ARG, "%s bilateral: radii %d, %d outside 0 .. %d", plane, p.rx, p.ry, HVQ_BIL_MAX_RADIUS);
    if (!p.spatial[0][0] || !p.range[0]) return fail(HVQ_E_ARG, "%s bilateral: spatial[0][0] %d, range[0] %d (the centre tap has a weight: both at least 1)", plane, p.spatial[0][0], p.range[0]);
    if (p.pad[0] || p.pad[1]) return fail(HVQ_E_ARG, "%s bilateral: pad %d, %d (0)", plane, p.pad[0], p.pad[1]);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_bilateral_check(const HvqBilateral *b)
{
    if (!b) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = bilateral_plane_check(b->luma, "luma"); if (rc) return rc; }
    return bilateral_plane_check(b->chroma, "chroma");
}

HVQ_EXPORT int hvq_bilateral_force_general(HvqContext *c, int on) { return force_switch(c, &HvqContext::bl_force_general, on); }

HVQ_EXPORT int hvq_bilateral_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                      const HvqMetricsRef *guide, const HvqBilateral *sets, int nsets, const int *which,
                                      void *const *dst, void *hip_stream)
{
    static_assert(HVQ_BIL_MAX_RADIUS == (int)HVQ_BL_MAX_R && HVQ_BIL_MAX_SETS == (int)HVQ_BL_MAX_SETS && sizeof(HvqBilateralPlane) == HVQ_BL_PLANE_BYTES &&
                  offsetof(HvqBilateralPlane, spatial) == HVQ_BL_SPATIAL_AT && offsetof(HvqBilateralPlane, range) == HVQ_BL_RANGE_AT &&
                  sizeof(HvqBilateral) == 2u * HVQ_BL_PLANE_BYTES, "the header's values and layout are the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst || !sets))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nsets < 1 || nsets > HVQ_BIL_MAX_SETS) return fail(HVQ_E_ARG, "%d sets: one call takes 1 .. %d", nsets, HVQ_BIL_MAX_SETS);
    for (int b = 0; b < nsets; ++b) { int rc = hvq_bilateral_check(sets + b); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, guide); if (rc) return rc; }
    const size_t job_bytes = (size_t)n * 3u * sizeof(HvqBilateralJob);
    std::vector<uint8_t> up(job_bytes + (size_t)nsets * sizeof(HvqBilateral));
    HvqBilateralJob *jobs = (HvqBilateralJob *)up.data();
    memcpy(up.data() + job_bytes, sets, (size_t)nsets * sizeof(HvqBilateral));
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr, *g = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        { int rc = picture_reference(c, i, streams[i], guide ? guide + i : nullptr, nullptr, &g); if (rc) return rc; }     /* null: the picture guides itself */
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("destination", i, dst[i]); if (rc) return rc; }
        const int b = which ? which[i] : 0;
        if (b < 0 || b >= nsets) return fail(HVQ_E_ARG, "picture %d: set %d of %d", i, b, nsets);
        uint8_t *const d = (uint8_t *)dst[i];
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            const HvqBilateralPlane &bp = p ? sets[b].chroma : sets[b].luma;
            HvqBilateralJob &j = jobs[(size_t)i * 3u + (size_t)p];
            j = hvq_bl_job((uint64_t)(uintptr_t)(a + off), (uint64_t)(uintptr_t)(d + off), g ? (uint64_t)(uintptr_t)(g + off) : 0u, nx, ny,
                           (uint32_t)(2 * b + (p ? 1 : 0)), (uint32_t)bp.rx, (uint32_t)bp.ry, c->bl_force_general);
            return j.tiles;
        }));
    }
    return slot_enqueue(c, hvq_launch_bilateral, "bilateral", "hvq_bilateral.hip", up, n, max_tiles, hip_stream);
}

/* Lookup tables on resident pictures in slot layout (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "The slot-layout frame"):
 * a job holds the device address of its 256 table bytes, which are read when the launch runs */
HVQ_EXPORT int hvq_map_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                const uint8_t *tables, int ntables, const int *which, int planes, void *const *dst, void *hip_stream)
{
    static_assert(HVQ_MAP_TABLE_BYTES == 3 * 256, "a record is a table of 256 bytes per plane");
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (!tables || ((uintptr_t)tables & 15u)) return fail(HVQ_E_ARG, "tables must be a non-null multiple of 16");
    if (ntables < 1 || ntables > 65535) return fail(HVQ_E_ARG, "%d tables: one call takes 1 .. 65535", ntables);
    if (!which && ntables != 1 && ntables != n) return fail(HVQ_E_ARG, "%d tables for %d pictures without `which` (1, or one per picture)", ntables, n);
    if (planes < 1 || planes > 7) return fail(HVQ_E_ARG, "planes %d: a mask of the bits 0 .. 2, not 0", planes);
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqMapJob> jobs((size_t)n * 3u);
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("destination", i, dst[i]); if (rc) return rc; }
        const int r = which ? which[i] : ntables == 1 ? 0 : i;
        if (r < 0 || r >= ntables) return fail(HVQ_E_ARG, "picture %d: table %d of %d", i, r, ntables);
        uint8_t *const b = (uint8_t *)dst[i];
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            HvqMapJob &j = jobs[(size_t)i * 3u + (size_t)p];
            j = hvq_mp_job((uint64_t)(uintptr_t)(a + off), (uint64_t)(uintptr_t)(b + off),
                           (uint64_t)(uintptr_t)(tables + (size_t)r * HVQ_MAP_TABLE_BYTES + 256u * (size_t)p), nx, ny, (planes >> p) & 1);
            return j.tiles;
        }));
    }
    return slot_enqueue(c, hvq_launch_map, "map", "hvq_map.hip", jobs, n, max_tiles, hip_stream);
}

/* Connected components of resident pictures (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "Labels").  The launches of a call
 * go behind ONE job table; the label map is the only working memory. */
HVQ_EXPORT int hvq_label_check(const HvqLabelRule *r)
{
    if (!r) return fail(HVQ_E_ARG, "bad arguments");
    if (r->plane < 0 || r->plane > 2) return fail(HVQ_E_ARG, "label rule: plane %d (0 Y, 1 U, 2 V)", r->plane);
    if (r->lo < 0 || r->lo > r->hi || r->hi > 255) return fail(HVQ_E_ARG, "label rule: window %d .. %d (0 <= lo <= hi <= 255)", r->lo, r->hi);
    if (r->connectivity != 4 && r->connectivity != 8) return fail(HVQ_E_ARG, "label rule: connectivity %d (4 or 8)", r->connectivity);
    return HVQ_OK;
}

HVQ_EXPORT int64_t hvq_label_bytes(int width, int height, int h_samp, int v_samp, int plane)
{
    { int rc = geometry_supported(width, height, h_samp, v_samp); if (rc) return rc; }
    if (plane < 0 || plane > 2) return fail(HVQ_E_ARG, "plane %d (0 Y, 1 U, 2 V)", plane);
    const SlotShape s = slot_shape(width, height, h_samp, v_samp);
    return 4 * (int64_t)(s.w >> (plane ? s.xs : 0)) * (int64_t)(s.h >> (plane ? s.ys : 0));
}

HVQ_EXPORT int hvq_label_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                  const HvqLabelRule *rules, int nrules, const int *which, uint32_t *const *labels, uint64_t *const *comps,
                                  int cap, void *hip_stream)
{
    static_assert(HVQ_LBL_INCOMPLETE == (int)HVQ_LB_INCOMPLETE, "the header's value is the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !labels || !comps || !rules))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nrules < 1 || nrules > HVQ_LBL_MAX_RULES) return fail(HVQ_E_ARG, "%d rules: one call takes 1 .. %d", nrules, HVQ_LBL_MAX_RULES);
    for (int r = 0; r < nrules; ++r) { int rc = hvq_label_check(rules + r); if (rc) return rc; }
    if (cap < 0 || cap > HVQ_LBL_MAX_CAP) return fail(HVQ_E_ARG, "cap %d outside 0 .. %d", cap, HVQ_LBL_MAX_CAP);
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqLabelJob> jobs((size_t)n);
    uint32_t max_tiles = 0, max_seams = 0, max_chunks = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("label map", i, labels[i]); if (rc) return rc; }
        { int rc = slot_pointer_check("record table", i, comps[i]); if (rc) return rc; }
        const int r = which ? which[i] : 0;
        if (r < 0 || r >= nrules) return fail(HVQ_E_ARG, "picture %d: rule %d of %d", i, r, nrules);
        const HvqLabelRule &rule = rules[r];
        HvqLabelJob &j = jobs[(size_t)i];
        plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            if (p == rule.plane)
                j = hvq_lb_job((uint64_t)(uintptr_t)(a + off), (uint64_t)(uintptr_t)labels[i], (uint64_t)(uintptr_t)comps[i], nx, ny,
                               (uint32_t)rule.lo, (uint32_t)rule.hi, (uint32_t)rule.connectivity, (uint32_t)cap);
            return 0;
        });
        max_tiles = std::max(max_tiles, j.tx * j.ty);
        max_seams = std::max(max_seams, j.seams);
        max_chunks = std::max(max_chunks, j.chunks);
    }
    { int rc = kernel_check(hvq_launch_label, "label", "hvq_label.hip", true); if (rc) return rc; }
    return export_enqueue(c, jobs.data(), jobs.size() * sizeof(HvqLabelJob), hip_stream,
                          [=](const void *t, hipStream_t st) { return hvq_launch_label(t, n, max_tiles, max_seams, max_chunks, st); });
}

/* Labels and records back into mask pictures in slot layout.  No picture is looked up: the stream gives the geometry; the launch goes
 * behind its job table through export_enqueue, so it is ordered behind an hvq_label_pictures on the same stream. */
HVQ_EXPORT int hvq_select_components(HvqContext *c, int n, const int *streams, const uint32_t *const *labels, const uint64_t *const *comps,
                                     int cap, const HvqSelect *sel, int nsel, const int *which, void *const *dst, void *hip_stream)
{
    if (!c || n < 0 || (n && (!streams || !labels || !comps || !sel || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nsel < 1 || nsel > HVQ_SEL_MAX) return fail(HVQ_E_ARG, "%d selections: one call takes 1 .. %d", nsel, HVQ_SEL_MAX);
    for (int k = 0; k < nsel; ++k) {
        const HvqSelect &e = sel[k];
        if (e.area_min > e.area_max || e.w_min > e.w_max || e.h_min > e.h_max) return fail(HVQ_E_ARG, "selection %d: a range with min above max", k);
        if (e.invert > 1u || e.pad) return fail(HVQ_E_ARG, "selection %d: invert %u, pad %u (0 or 1; 0)", k, e.invert, e.pad);
    }
    if (cap < 0 || cap > HVQ_LBL_MAX_CAP) return fail(HVQ_E_ARG, "cap %d outside 0 .. %d", cap, HVQ_LBL_MAX_CAP);
    std::vector<HvqSelectJob> jobs((size_t)n * 3u);
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || (size_t)streams[i] >= c->streams.size() || !c->streams[(size_t)streams[i]].open) return fail(HVQ_E_ARG, "bad stream %d", streams[i]);
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("label map", i, labels[i]); if (rc) return rc; }
        { int rc = slot_pointer_check("record table", i, comps[i]); if (rc) return rc; }
        { int rc = slot_pointer_check("destination", i, dst[i]); if (rc) return rc; }
        const int k = which ? which[i] : 0;
        if (k < 0 || k >= nsel) return fail(HVQ_E_ARG, "picture %d: selection %d of %d", i, k, nsel);
        const uint32_t range[6] = { sel[k].area_min, sel[k].area_max, sel[k].w_min, sel[k].w_max, sel[k].h_min, sel[k].h_max };
        uint8_t *const b = (uint8_t *)dst[i];
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            HvqSelectJob &j = jobs[(size_t)i * 3u + (size_t)p];
            j = hvq_sl_job((uint64_t)(uintptr_t)labels[i], (uint64_t)(uintptr_t)comps[i], (uint64_t)(uintptr_t)(b + off), nx, ny, (uint32_t)cap, p == 0,
                           range, sel[k].invert);
            return j.tiles;
        }));
    }
    HIPCHK(hipSetDevice(c->device));
    return slot_enqueue(c, hvq_launch_select, "select", "hvq_label.hip", jobs, n, max_tiles, hip_stream);
}

/* Corners of resident pictures (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "Corners").  The four launches of a call go
 * behind ONE job table; there is no memory besides the outputs. */
HVQ_EXPORT int hvq_corner_check(const HvqCornerRule *r)
{
    if (!r) return fail(HVQ_E_ARG, "bad arguments");
    if (r->plane < 0 || r->plane > 2) return fail(HVQ_E_ARG, "corner rule: plane %d (0 Y, 1 U, 2 V)", r->plane);
    if (r->mode != HVQ_CRN_HARRIS && r->mode != HVQ_CRN_MIN_EIGEN) return fail(HVQ_E_ARG, "corner rule: mode %d (0 Harris, 1 min-eigenvalue)", r->mode);
    if (r->radius < 1 || r->radius > HVQ_CRN_MAX_RADIUS) return fail(HVQ_E_ARG, "corner rule: radius %d outside 1 .. %d", r->radius, HVQ_CRN_MAX_RADIUS);
    if (r->k < 0 || r->k > 64 || (r->mode == HVQ_CRN_MIN_EIGEN && r->k)) return fail(HVQ_E_ARG, "corner rule: k %d (0 .. 64 under Harris, 0 under min-eigenvalue)", r->k);
    if (r->nms < 0 || r->nms > HVQ_CRN_MAX_NMS) return fail(HVQ_E_ARG, "corner rule: nms %d outside 0 .. %d", r->nms, HVQ_CRN_MAX_NMS);
    if (r->margin < 0 || r->margin > 255) return fail(HVQ_E_ARG, "corner rule: margin %d outside 0 .. 255", r->margin);
    if (r->threshold < 1) return fail(HVQ_E_ARG, "corner rule: threshold %lld (at least 1)", (long long)r->threshold);
    if (r->pad[0] || r->pad[1]) return fail(HVQ_E_ARG, "corner rule: pad %d, %d (0)", r->pad[0], r->pad[1]);
    return HVQ_OK;
}

static int corner_plane(int width, int height, int h_samp, int v_samp, int plane, int64_t *nx, int64_t *ny)
{
    { int rc = geometry_supported(width, height, h_samp, v_samp); if (rc) return rc; }
    if (plane < 0 || plane > 2) return fail(HVQ_E_ARG, "plane %d (0 Y, 1 U, 2 V)", plane);
    const SlotShape s = slot_shape(width, height, h_samp, v_samp);
    *nx = s.w >> (plane ? s.xs : 0); *ny = s.h >> (plane ? s.ys : 0);
    return HVQ_OK;
}

HVQ_EXPORT int64_t hvq_corner_rows_bytes(int width, int height, int h_samp, int v_samp, int plane)
{
    int64_t nx = 0, ny = 0;
    { int rc = corner_plane(width, height, h_samp, v_samp, plane, &nx, &ny); if (rc) return rc; }
    return 4 * (ny + 1);
}

HVQ_EXPORT int64_t hvq_corner_response_bytes(int width, int height, int h_samp, int v_samp, int plane)
{
    int64_t nx = 0, ny = 0;
    { int rc = corner_plane(width, height, h_samp, v_samp, plane, &nx, &ny); if (rc) return rc; }
    return 8 * nx * ny;
}

HVQ_EXPORT int hvq_corner_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                   const HvqCornerRule *rules, int nrules, const int *which, uint8_t *const *mask, int64_t *const *points,
                                   uint32_t *const *rows, int64_t *const *response, int cap, void *hip_stream)
{
    static_assert(HVQ_CRN_HARRIS == (int)HVQ_CR_HARRIS && HVQ_CRN_MIN_EIGEN == (int)HVQ_CR_MIN_EIGEN && HVQ_CRN_MAX_RADIUS == (int)HVQ_CR_MAX_R &&
                  HVQ_CRN_MAX_NMS == (int)HVQ_CR_MAX_NMS && sizeof(HvqCornerRule) == 40 && offsetof(HvqCornerRule, threshold) == 32,
                  "the header's values and layout are the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !mask || !points || !rows || !rules))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nrules < 1 || nrules > HVQ_CRN_MAX_RULES) return fail(HVQ_E_ARG, "%d rules: one call takes 1 .. %d", nrules, HVQ_CRN_MAX_RULES);
    for (int r = 0; r < nrules; ++r) { int rc = hvq_corner_check(rules + r); if (rc) return rc; }
    if (cap < 0 || cap > HVQ_CRN_MAX_CAP) return fail(HVQ_E_ARG, "cap %d outside 0 .. %d", cap, HVQ_CRN_MAX_CAP);
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqCornerJob> jobs((size_t)n);
    uint32_t max_tiles = 0, max_rows = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("mask", i, mask[i]); if (rc) return rc; }
        { int rc = slot_pointer_check("point list", i, points[i]); if (rc) return rc; }
        { int rc = slot_pointer_check("row index", i, rows[i]); if (rc) return rc; }
        int64_t *const resp = response ? response[i] : nullptr;
        if ((uintptr_t)resp & 15u) return fail(HVQ_E_ARG, "response map %d: the pointer must be a multiple of 16", i);
        const int r = which ? which[i] : 0;
        if (r < 0 || r >= nrules) return fail(HVQ_E_ARG, "picture %d: rule %d of %d", i, r, nrules);
        const HvqCornerRule &rule = rules[r];
        uint64_t off[3] = { 0, 0, 0 }, from = 0;
        uint32_t dw[3] = { 0, 0, 0 }, px = 0, py = 0;
        plane_walk(slot_shape(s), [&](int p, size_t o, uint32_t nx, uint32_t ny) {
            off[p] = o; dw[p] = (nx >> 2) * ny;
            if (p == rule.plane) { from = o; px = nx; py = ny; }
            return 0;
        });
        HvqCornerJob &j = jobs[(size_t)i];
        j = hvq_cr_job((uint64_t)(uintptr_t)(a + from), (uint64_t)(uintptr_t)mask[i], off, dw, (uint32_t)rule.plane, (uint64_t)(uintptr_t)points[i],
                       (uint64_t)(uintptr_t)rows[i], (uint64_t)(uintptr_t)resp, px, py, (uint32_t)rule.mode, (uint32_t)rule.radius, (uint32_t)rule.k,
                       (uint32_t)rule.nms, (uint32_t)rule.margin, rule.threshold, (uint32_t)cap);
        max_tiles = std::max(max_tiles, hvq_cr_tiles(j));
        max_rows = std::max(max_rows, j.ny);
    }
    { int rc = kernel_check(hvq_launch_corner, "corner", "hvq_corner.hip", true); if (rc) return rc; }
    return export_enqueue(c, jobs.data(), jobs.size() * sizeof(HvqCornerJob), hip_stream,
                          [=](const void *t, hipStream_t st) { return hvq_launch_corner(t, n, max_tiles, max_rows, st); });
}

/* Exact distance transforms of resident pictures (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "Distances").  The two launches
 * of a call go behind ONE job table; the map is the only working memory. */
HVQ_EXPORT int hvq_distance_check(const HvqDistanceRule *r)
{
    if (!r) return fail(HVQ_E_ARG, "bad arguments");
    if (r->plane < 0 || r->plane > 2) return fail(HVQ_E_ARG, "distance rule: plane %d (0 Y, 1 U, 2 V)", r->plane);
    if (r->lo < 0 || r->lo > r->hi || r->hi > 255) return fail(HVQ_E_ARG, "distance rule: window %d .. %d (0 <= lo <= hi <= 255)", r->lo, r->hi);
    if (r->metric < HVQ_DST_EUCLID2 || r->metric > HVQ_DST_CHESS) return fail(HVQ_E_ARG, "distance rule: metric %d (0 EUCLID2, 1 CITY, 2 CHESS)", r->metric);
    if (r->border < 0 || r->border > 1) return fail(HVQ_E_ARG, "distance rule: border %d (0 or 1)", r->border);
    if (r->pad[0] || r->pad[1] || r->pad[2]) return fail(HVQ_E_ARG, "distance rule: pad must be 0");
    return HVQ_OK;
}

HVQ_EXPORT int64_t hvq_distance_bytes(int width, int height, int h_samp, int v_samp, int plane)
{
    return hvq_label_bytes(width, height, h_samp, v_samp, plane);     /* a uint32 a sample, like a label map */
}

HVQ_EXPORT int hvq_distance_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                     const HvqDistanceRule *rules, int nrules, const int *which, uint32_t *const *dist, void *hip_stream)
{
    static_assert(HVQ_DST_EUCLID2 == (int)HVQ_DT_EUCLID2 && HVQ_DST_CITY == (int)HVQ_DT_CITY && HVQ_DST_CHESS == (int)HVQ_DT_CHESS && HVQ_DST_NONE == HVQ_DT_NONE,
                  "the header's values are the kernels'");
    if (!c || n < 0 || (n && (!streams || !ordinals || !dist || !rules))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nrules < 1 || nrules > HVQ_DST_MAX_RULES) return fail(HVQ_E_ARG, "%d rules: one call takes 1 .. %d", nrules, HVQ_DST_MAX_RULES);
    for (int r = 0; r < nrules; ++r) { int rc = hvq_distance_check(rules + r); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqDistanceJob> jobs((size_t)n);
    uint32_t max_cols = 0, max_rows = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("distance map", i, dist[i]); if (rc) return rc; }
        const int r = which ? which[i] : 0;
        if (r < 0 || r >= nrules) return fail(HVQ_E_ARG, "picture %d: rule %d of %d", i, r, nrules);
        const HvqDistanceRule &rule = rules[r];
        HvqDistanceJob &j = jobs[(size_t)i];
        plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            if (p == rule.plane)
                j = hvq_dt_job((uint64_t)(uintptr_t)(a + off), (uint64_t)(uintptr_t)dist[i], nx, ny, (uint32_t)rule.lo, (uint32_t)rule.hi, (uint32_t)rule.metric,
                               (uint32_t)rule.border);
            return 0;
        });
        if (j.nx > HVQ_DT_SPAN) return fail(HVQ_E_ARG, "picture %d: a row of %u samples, the row pass holds %u", i, j.nx, HVQ_DT_SPAN);
        max_cols = std::max(max_cols, j.colgroups);
        max_rows = std::max(max_rows, j.rowgroups);
    }
    { int rc = kernel_check(hvq_launch_distance, "distance", "hvq_distance.hip", true); if (rc) return rc; }
    return export_enqueue(c, jobs.data(), jobs.size() * sizeof(HvqDistanceJob), hip_stream,
                          [=](const void *t, hipStream_t st) { return hvq_launch_distance(t, n, max_cols, max_rows, st); });
}

/* Distances back into mask pictures in slot layout.  No picture is looked up: the stream gives the geometry; the launch goes behind its
 * job table through export_enqueue, so it is ordered behind an hvq_distance_pictures on the same stream. */
HVQ_EXPORT int hvq_distance_mask_check(const HvqDistanceMask *m)
{
    if (!m) return fail(HVQ_E_ARG, "bad arguments");
    if (m->mode > (uint32_t)HVQ_DSM_ROOT) return fail(HVQ_E_ARG, "distance mask: mode %u (0 RANGE, 1 ROOT)", m->mode);
    if (m->lo > m->hi) return fail(HVQ_E_ARG, "distance mask: range %u .. %u", m->lo, m->hi);
    if (m->invert > 1u) return fail(HVQ_E_ARG, "distance mask: invert %u (0 or 1)", m->invert);
    if (m->pad[0] || m->pad[1] || m->pad[2] || m->pad[3]) return fail(HVQ_E_ARG, "distance mask: pad must be 0");
    if (m->mode == (uint32_t)HVQ_DSM_ROOT && (m->lo || m->hi || m->invert)) return fail(HVQ_E_ARG, "distance mask: ROOT takes lo, hi and invert 0");
    return HVQ_OK;
}

HVQ_EXPORT int hvq_distance_mask(HvqContext *c, int n, const int *streams, const uint32_t *const *dist, const HvqDistanceMask *sel, int nsel,
                                 const int *which, void *const *dst, void *hip_stream)
{
    static_assert(HVQ_DSM_RANGE == (int)HVQ_DM_RANGE && HVQ_DSM_ROOT == (int)HVQ_DM_ROOT, "the header's values are the kernel's");
    if (!c || n < 0 || (n && (!streams || !dist || !sel || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nsel < 1 || nsel > HVQ_DSM_MAX) return fail(HVQ_E_ARG, "%d masks: one call takes 1 .. %d", nsel, HVQ_DSM_MAX);
    for (int k = 0; k < nsel; ++k) { int rc = hvq_distance_mask_check(sel + k); if (rc) return rc; }
    std::vector<HvqDistMaskJob> jobs((size_t)n * 3u);
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || (size_t)streams[i] >= c->streams.size() || !c->streams[(size_t)streams[i]].open) return fail(HVQ_E_ARG, "bad stream %d", streams[i]);
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("distance map", i, dist[i]); if (rc) return rc; }
        { int rc = slot_pointer_check("destination", i, dst[i]); if (rc) return rc; }
        const int k = which ? which[i] : 0;
        if (k < 0 || k >= nsel) return fail(HVQ_E_ARG, "picture %d: mask %d of %d", i, k, nsel);
        uint8_t *const b = (uint8_t *)dst[i];
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            HvqDistMaskJob &j = jobs[(size_t)i * 3u + (size_t)p];
            j = hvq_dm_job((uint64_t)(uintptr_t)dist[i], (uint64_t)(uintptr_t)(b + off), nx, ny, p ? HVQ_DM_FILL : sel[k].mode, sel[k].lo, sel[k].hi, sel[k].invert);
            return j.tiles;
        }));
    }
    HIPCHK(hipSetDevice(c->device));
    return slot_enqueue(c, hvq_launch_distance_mask, "distance mask", "hvq_distance.hip", jobs, n, max_tiles, hip_stream);
}

/* Summed-area tables of resident pictures (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "Integrals").  The two launches of a
 * call go behind ONE job table; the tables are the only working memory. */
HVQ_EXPORT int64_t hvq_integral_bytes(int width, int height, int h_samp, int v_samp, int plane, int order)
{
    if (order != 1 && order != 2) return fail(HVQ_E_ARG, "order %d (1 sums, 2 squares)", order);
    const int64_t b = hvq_label_bytes(width, height, h_samp, v_samp, plane);    /* a uint32 a sample */
    return b < 0 ? b : b * order;
}

HVQ_EXPORT int hvq_integral_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src, const int *which_plane,
                                     uint32_t *const *sums, uint64_t *const *squares, void *hip_stream)
{
    if (!c || n < 0 || (n && (!streams || !ordinals || !sums))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqIntegralJob> jobs((size_t)n);
    uint32_t max_rows = 0, max_cols = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("table of sums", i, sums[i]); if (rc) return rc; }
        uint64_t *const q = squares ? squares[i] : nullptr;
        if ((uintptr_t)q & 15u) return fail(HVQ_E_ARG, "table of squares %d: the pointer must be a multiple of 16", i);
        const int plane = which_plane ? which_plane[i] : 0;
        if (plane < 0 || plane > 2) return fail(HVQ_E_ARG, "picture %d: plane %d (0 Y, 1 U, 2 V)", i, plane);
        HvqIntegralJob &j = jobs[(size_t)i];
        plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            if (p == plane) j = hvq_ig_job((uint64_t)(uintptr_t)(a + off), (uint64_t)(uintptr_t)sums[i], (uint64_t)(uintptr_t)q, nx, ny);
            return 0;
        });
        max_rows = std::max(max_rows, j.rowgroups);
        max_cols = std::max(max_cols, j.colgroups);
    }
    { int rc = kernel_check(hvq_launch_integral, "integral", "hvq_integral.hip", true); if (rc) return rc; }
    return export_enqueue(c, jobs.data(), jobs.size() * sizeof(HvqIntegralJob), hip_stream,
                          [=](const void *t, hipStream_t st) { return hvq_launch_integral(t, n, max_rows, max_cols, st); });
}

/* Tables back into pictures in slot layout: local means, deviations, thresholds.  The launch goes behind its job table through
 * export_enqueue, so it is ordered behind an hvq_integral_pictures on the same stream. */
HVQ_EXPORT int hvq_window_check(const HvqWindowRule *r)
{
    if (!r) return fail(HVQ_E_ARG, "bad arguments");
    if (r->plane < 0 || r->plane > 2) return fail(HVQ_E_ARG, "window rule: plane %d (0 Y, 1 U, 2 V)", r->plane);
    if (r->mode < HVQ_WIN_MEAN || r->mode > HVQ_WIN_THRESHOLD) return fail(HVQ_E_ARG, "window rule: mode %d (0 MEAN, 1 DEVIATION, 2 THRESHOLD)", r->mode);
    if (r->rx < 0 || r->rx > HVQ_WIN_MAX_RADIUS || r->ry < 0 || r->ry > HVQ_WIN_MAX_RADIUS)
        return fail(HVQ_E_ARG, "window rule: radii %d, %d (0 .. %d)", r->rx, r->ry, HVQ_WIN_MAX_RADIUS);
    if (r->k < -1024 || r->k > 1024) return fail(HVQ_E_ARG, "window rule: k %d (-1024 .. 1024)", r->k);
    if (r->c < -255 || r->c > 255) return fail(HVQ_E_ARG, "window rule: c %d (-255 .. 255)", r->c);
    if (r->invert < 0 || r->invert > 1) return fail(HVQ_E_ARG, "window rule: invert %d (0 or 1)", r->invert);
    if (r->pad) return fail(HVQ_E_ARG, "window rule: pad must be 0");
    return HVQ_OK;
}

HVQ_EXPORT int hvq_window_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src, const uint32_t *const *sums,
                                   const uint64_t *const *squares, const HvqWindowRule *rules, int nrules, const int *which, void *const *dst, void *hip_stream)
{
    static_assert(HVQ_WIN_MEAN == (int)HVQ_WN_MEAN && HVQ_WIN_DEVIATION == (int)HVQ_WN_DEVIATION && HVQ_WIN_THRESHOLD == (int)HVQ_WN_THRESHOLD,
                  "the header's values are the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !sums || !rules || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (nrules < 1 || nrules > HVQ_WIN_MAX_RULES) return fail(HVQ_E_ARG, "%d rules: one call takes 1 .. %d", nrules, HVQ_WIN_MAX_RULES);
    for (int r = 0; r < nrules; ++r) { int rc = hvq_window_check(rules + r); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqWindowJob> jobs((size_t)n);
    uint32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        { int rc = slot_pointer_check("table of sums", i, sums[i]); if (rc) return rc; }
        { int rc = slot_pointer_check("destination", i, dst[i]); if (rc) return rc; }
        const uint64_t *const q = squares ? squares[i] : nullptr;
        if ((uintptr_t)q & 15u) return fail(HVQ_E_ARG, "table of squares %d: the pointer must be a multiple of 16", i);
        const int r = which ? which[i] : 0;
        if (r < 0 || r >= nrules) return fail(HVQ_E_ARG, "picture %d: rule %d of %d", i, r, nrules);
        const HvqWindowRule &rule = rules[r];
        if (!q && hvq_wn_needs_squares((uint32_t)rule.mode, rule.k)) return fail(HVQ_E_ARG, "picture %d: rule %d needs the table of squares", i, r);
        size_t plane_off = 0;
        uint32_t pnx = 0, pny = 0, ynx = 0, yny = 0, cdwords = 0;
        plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            if (!p) { ynx = nx; yny = ny; } else cdwords += (nx * ny) >> 2;
            if (p == rule.plane) { plane_off = off; pnx = nx; pny = ny; }
            return 0;
        });
        if (pnx != ynx || pny != yny) return fail(HVQ_E_ARG, "picture %d: plane %d is %u x %u, Y %u x %u: the result is written into Y", i, rule.plane, pnx, pny, ynx, yny);
        const uint64_t wx = std::min<uint64_t>(2u * (uint64_t)rule.rx + 1u, ynx), wy = std::min<uint64_t>(2u * (uint64_t)rule.ry + 1u, yny);
        if (wx * wy > HVQ_WN_MAX_AREA) return fail(HVQ_E_ARG, "picture %d: a window of %llu x %llu samples, a window holds 2^24", i, (unsigned long long)wx, (unsigned long long)wy);
        HvqWindowJob &j = jobs[(size_t)i];
        j = hvq_wn_job((uint64_t)(uintptr_t)(a + plane_off), (uint64_t)(uintptr_t)sums[i], (uint64_t)(uintptr_t)q, (uint64_t)(uintptr_t)dst[i], ynx, yny, cdwords,
                       (uint32_t)rule.mode, (uint32_t)rule.rx, (uint32_t)rule.ry, rule.k, rule.c, (uint32_t)rule.invert);
        max_tiles = std::max(max_tiles, j.tiles);
    }
    return slot_enqueue(c, hvq_launch_window, "window", "hvq_integral.hip", jobs, n, max_tiles, hip_stream);
}

/* Sums of rectangles that lie in device memory.  No picture is looked up; ONE head and a pair of tables a picture go up as the job table */
HVQ_EXPORT int hvq_rect_sums(HvqContext *c, int n, int nrects, const int32_t *rects, const uint32_t *const *sums, const uint64_t *const *squares, const uint32_t *dims,
                             uint64_t *out, void *hip_stream)
{
    if (!c || n < 0 || nrects < 0 || !sums) return fail(HVQ_E_ARG, "bad arguments");
    if (n < 1) return fail(HVQ_E_ARG, "%d pictures: one call takes 1 .. 65535", n);
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (nrects > HVQ_RECT_MAX) return fail(HVQ_E_ARG, "%d rectangles: one call takes %d at the most", nrects, HVQ_RECT_MAX);
    if (!nrects) return HVQ_OK;
    if (!rects || ((uintptr_t)rects & 3u) || !dims || ((uintptr_t)dims & 3u) || !out || ((uintptr_t)out & 7u))
        return fail(HVQ_E_ARG, "rects and dims must be non-null multiples of 4, out a non-null multiple of 8");
    std::vector<HvqRectTables> tab((size_t)n + 2u);                    /* the head takes the room of two */
    static_assert(sizeof(HvqRectHead) == 2 * sizeof(HvqRectTables), "the head lies before the tables");
    HvqRectHead head = { (uint64_t)(uintptr_t)rects, (uint64_t)(uintptr_t)dims, (uint64_t)(uintptr_t)out, (uint32_t)nrects, (uint32_t)n };
    memcpy(tab.data(), &head, sizeof head);
    for (int i = 0; i < n; ++i) {
        { int rc = slot_pointer_check("table of sums", i, sums[i]); if (rc) return rc; }
        const uint64_t *const q = squares ? squares[i] : nullptr;
        if ((uintptr_t)q & 15u) return fail(HVQ_E_ARG, "table of squares %d: the pointer must be a multiple of 16", i);
        tab[(size_t)i + 2u] = HvqRectTables{ (uint64_t)(uintptr_t)sums[i], (uint64_t)(uintptr_t)q };
    }
    HIPCHK(hipSetDevice(c->device));
    return slot_enqueue(c, hvq_launch_rects, "rectangle", "hvq_integral.hip", tab, n, (uint32_t)nrects, hip_stream);
}

/* Tables from histogram records (include/hvqm4_amd.h: the specification).  No picture is looked up; the launch goes behind its job
 * table through export_enqueue like the chain's members, so it is ordered behind an hvq_picture_histograms on the same stream. */
static int table_plane_check(const HvqTablePlane &p, const char *plane)
{
    if (p.kind < HVQ_TBL_IDENTITY || p.kind > HVQ_TBL_OTSU) return fail(HVQ_E_ARG, "%s table: kind %d", plane, p.kind);
    if (p.pad) return fail(HVQ_E_ARG, "%s table: pad %d (0)", plane, p.pad);
    if (p.kind == HVQ_TBL_FLAT) {
        if (p.a < 0 || p.a > 255 || p.b) return fail(HVQ_E_ARG, "%s table: FLAT with a %d, b %d (a in 0 .. 255, b 0)", plane, p.a, p.b);
    } else if (p.kind == HVQ_TBL_STRETCH) {
        if (p.a < 0 || p.a > 499 || p.b < 0 || p.b > 499) return fail(HVQ_E_ARG, "%s table: STRETCH with clips %d, %d outside 0 .. 499", plane, p.a, p.b);
    } else if (p.a || p.b) {
        return fail(HVQ_E_ARG, "%s table: kind %d takes no a, b (%d, %d)", plane, p.kind, p.a, p.b);
    }
    return HVQ_OK;
}

HVQ_EXPORT int hvq_table_check(const HvqTableRule *r)
{
    if (!r) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = table_plane_check(r->luma, "luma"); if (rc) return rc; }
    return table_plane_check(r->chroma, "chroma");
}

HVQ_EXPORT int hvq_histogram_tables(HvqContext *c, int n, const uint32_t *hist, const HvqTableRule *rules, int nrules, const int *which,
                                    uint8_t *tables, void *hip_stream)
{
    static_assert(HVQ_TBL_IDENTITY == (int)HVQ_TB_IDENTITY && HVQ_TBL_FLAT == (int)HVQ_TB_FLAT && HVQ_TBL_EQUALIZE == (int)HVQ_TB_EQUALIZE &&
                  HVQ_TBL_STRETCH == (int)HVQ_TB_STRETCH && HVQ_TBL_OTSU == (int)HVQ_TB_OTSU, "the header's values are the kernel's");
    if (!c || n < 0) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "records"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    if (!hist || ((uintptr_t)hist & 15u) || !tables || ((uintptr_t)tables & 15u)) return fail(HVQ_E_ARG, "hist and tables must be non-null multiples of 16");
    if (!rules || nrules < 1 || nrules > HVQ_TBL_MAX_RULES) return fail(HVQ_E_ARG, "%d rules: one call takes 1 .. %d", rules ? nrules : 0, HVQ_TBL_MAX_RULES);
    for (int r = 0; r < nrules; ++r) { int rc = hvq_table_check(rules + r); if (rc) return rc; }
    std::vector<HvqTableJob> jobs((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int r = which ? which[i] : 0;
        if (r < 0 || r >= nrules) return fail(HVQ_E_ARG, "record %d: rule %d of %d", i, r, nrules);
        HvqTableJob &j = jobs[(size_t)i];
        j.hist = (uint64_t)(uintptr_t)(hist + (size_t)i * 3u * HVQ_HIST_BINS);
        j.out = (uint64_t)(uintptr_t)(tables + (size_t)i * HVQ_MAP_TABLE_BYTES);
        const HvqTablePlane *pl[2] = { &rules[r].luma, &rules[r].chroma };
        for (int k = 0; k < 2; ++k) { j.rule[k].kind = (uint32_t)pl[k]->kind; j.rule[k].a = (uint32_t)pl[k]->a; j.rule[k].b = (uint32_t)pl[k]->b; j.rule[k].pad = 0; }
    }
    { int rc = kernel_check(hvq_launch_tables, "table", "hvq_map.hip"); if (rc) return rc; }
    HIPCHK(hipSetDevice(c->device));
    return export_enqueue(c, jobs.data(), jobs.size() * sizeof(HvqTableJob), hip_stream,
                          [=](const void *t, hipStream_t st) { return hvq_launch_tables(t, n, st); });
}

/* Warped copies of resident pictures in slot layout (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "The slot-layout frame") */
HVQ_EXPORT int hvq_warp_check(const HvqWarp *w)
{
    if (!w) return fail(HVQ_E_ARG, "bad arguments");
    const int32_t m[4] = { w->m00, w->m01, w->m10, w->m11 };
    for (int i = 0; i < 4; ++i)
        if (m[i] > HVQ_WARP_MAX_SCALE || m[i] < -HVQ_WARP_MAX_SCALE) return fail(HVQ_E_ARG, "warp: m%d%d = %d beyond %d", i >> 1, i & 1, m[i], HVQ_WARP_MAX_SCALE);
    if (w->border != HVQ_WARP_REPLICATE && w->border != HVQ_WARP_CONSTANT) return fail(HVQ_E_ARG, "warp: border %d", w->border);
    if (w->pad) return fail(HVQ_E_ARG, "warp: pad %d is not 0", w->pad);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_warp_body(const HvqWarp *w, int dst_h, int dst_v, int src_h, int src_v, int nx, int ny)
{
    { int rc = hvq_warp_check(w); if (rc) return rc; }
    if ((dst_h != 1 && dst_h != 2) || (dst_v != 1 && dst_v != 2) || (src_h != 1 && src_h != 2) || (src_v != 1 && src_v != 2))
        return fail(HVQ_E_ARG, "samplings %d x %d -> %d x %d: each is 1 or 2", src_h, src_v, dst_h, dst_v);
    if (nx < 1 || ny < 1 || nx > 8192 || ny > 8192) return fail(HVQ_E_ARG, "%d x %d: a plane has 1 .. 8192 samples a side", nx, ny);
    const int32_t m[6] = { w->m00, w->m01, w->m10, w->m11, w->t0, w->t1 };
    return (int)hvq_wp_job(0, 0, (uint32_t)nx, (uint32_t)ny, 8, 8, m, w->border, 0, dst_h, dst_v, src_h, src_v, 0).body;
}

HVQ_EXPORT int hvq_warp_force_direct(HvqContext *c, int on) { return force_switch(c, &HvqContext::wp_force, on, 3); }

HVQ_EXPORT int hvq_warp_pictures(HvqContext *c, int n, const int *streams, const int *ordinals, const void *const *src,
                                 const HvqWarp *warps, const HvqWarpDst *dst, void *hip_stream)
{
    static_assert(HVQ_WARP_DIRECT == (int)HVQ_WP_DIRECT && HVQ_WARP_TILED == (int)HVQ_WP_TILED && HVQ_WARP_MAX_SCALE == HVQ_WP_MAX_M,
                  "the header's names are the kernel's");
    if (!c || n < 0 || (n && (!streams || !ordinals || !dst || !warps))) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(n, "pictures"); if (rc) return rc; }
    if (!n) return HVQ_OK;
    for (int i = 0; i < n; ++i) { int rc = hvq_warp_check(warps + i); if (rc) return rc; }
    { int rc = chain_begin(c, n, streams, ordinals, src, nullptr); if (rc) return rc; }
    std::vector<HvqWarpJob> jobs((size_t)n * 3u);
    uint32_t max_tiles = 0;
    TargetSeen seen;
    for (int i = 0; i < n; ++i) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        const HvqWarpDst &d = dst[i];
        { int rc = slot_pointer_check("destination", i, d.ptr); if (rc) return rc; }
        { int rc = seen.check(d.width, d.height, d.h_samp, d.v_samp); if (rc) return rc; }
        const HvqWarp &w = warps[i];
        const int32_t m[6] = { w.m00, w.m01, w.m10, w.m11, w.t0, w.t1 };
        const SlotShape from = slot_shape(s), to = slot_shape(d.width, d.height, d.h_samp, d.v_samp);
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(from, to, [&](int p, size_t so, size_t dof, uint32_t nx, uint32_t ny, uint32_t mx, uint32_t my) {
            const int xs = p ? from.xs : 0, ys = p ? from.ys : 0, xd = p ? to.xs : 0, yd = p ? to.ys : 0;
            HvqWarpJob &j = jobs[(size_t)i * 3u + (size_t)p];
            j = hvq_wp_job((uint64_t)(uintptr_t)(a + so), (uint64_t)(uintptr_t)((uint8_t *)d.ptr + dof), nx, ny, mx, my, m, w.border, w.fill[p],
                           1 << xd, 1 << yd, 1 << xs, 1 << ys, c->wp_force);
            return j.tiles;
        }));
    }
    return slot_enqueue(c, hvq_launch_warp, "warp", "hvq_warp.hip", jobs, n, max_tiles, hip_stream);
}

/* Pictures composed of layers of resident pictures, in slot layout (include/hvqm4_amd.h: the specification; DESIGN.md 4.5, "The
 * slot-layout frame"): the chain's pictures are the flat layer sources; behind three jobs a target go three records a layer, the
 * rectangles of both sides in samples of the plane */
HVQ_EXPORT int hvq_compose_check(const HvqComposeLayer *l)
{
    if (!l) return fail(HVQ_E_ARG, "bad arguments");
    if (l->mode != HVQ_CMP_PUT && l->mode != HVQ_CMP_ADD) return fail(HVQ_E_ARG, "layer: mode %d", l->mode);
    if (l->sx < 0 || l->sy < 0 || l->w < 0 || l->h < 0 || l->dx < 0 || l->dy < 0)
        return fail(HVQ_E_ARG, "layer: a negative number in %d, %d, %d x %d -> %d, %d", l->sx, l->sy, l->w, l->h, l->dx, l->dy);
    if (l->w == 0 && (l->sx || l->sy || l->h)) return fail(HVQ_E_ARG, "layer: w == 0 means the whole source and takes sx, sy and h as 0");
    if (l->w > 0 && l->h == 0) return fail(HVQ_E_ARG, "layer: the rectangle %d x %d is empty", l->w, l->h);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_compose_force_general(HvqContext *c, int on) { return force_switch(c, &HvqContext::cp_force_general, on); }

HVQ_EXPORT int hvq_compose_pictures(HvqContext *c, int nlayers, const int *streams, const int *ordinals, const void *const *src,
                                    const HvqComposeLayer *layers, int ntargets, const HvqComposeDst *dst, void *hip_stream)
{
    static_assert(HVQ_CMP_PUT == (int)HVQ_CP_PUT && HVQ_CMP_ADD == (int)HVQ_CP_ADD && HVQ_CMP_MAX_GAIN == HVQ_CP_MAX_GAIN && HVQ_CMP_MAX_SHIFT < 31,
                  "the header's names are the kernel's");
    if (!c || nlayers < 0 || ntargets < 0 || (nlayers && (!streams || !ordinals || !layers)) || (ntargets && !dst)) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = count_check(ntargets, "targets"); if (rc) return rc; }
    if (nlayers > HVQ_CMP_MAX_TOTAL) return fail(HVQ_E_ARG, "%d layers: one call takes %d at the most", nlayers, HVQ_CMP_MAX_TOTAL);
    if (!ntargets) return HVQ_OK;
    for (int l = 0; l < nlayers; ++l) { int rc = hvq_compose_check(layers + l); if (rc) return rc; }
    TargetSeen seen;
    for (int t = 0; t < ntargets; ++t) {
        const HvqComposeDst &d = dst[t];
        { int rc = slot_pointer_check("target", t, d.ptr); if (rc) return rc; }
        { int rc = seen.check(d.width, d.height, d.h_samp, d.v_samp); if (rc) return rc; }
        if (d.shift < 0 || d.shift > HVQ_CMP_MAX_SHIFT) return fail(HVQ_E_ARG, "target %d: shift %d outside 0 .. %d", t, d.shift, HVQ_CMP_MAX_SHIFT);
        for (int p = 0; p < 3; ++p)
            if (d.bias[p] < -255 || d.bias[p] > 255) return fail(HVQ_E_ARG, "target %d: bias %d outside -255 .. 255", t, d.bias[p]);
        if (d.first < 0 || d.count < 0 || d.first > nlayers || d.count > nlayers - d.first)
            return fail(HVQ_E_ARG, "target %d: layers %d .. %d + %d of %d", t, d.first, d.first, d.count, nlayers);
        if (d.count > HVQ_CMP_MAX_LAYERS) return fail(HVQ_E_ARG, "target %d: %d layers, a target takes %d at the most", t, d.count, HVQ_CMP_MAX_LAYERS);
    }
    { int rc = chain_begin(c, nlayers, streams, ordinals, src, nullptr); if (rc) return rc; }
    const size_t job_bytes = (size_t)ntargets * 3u * sizeof(HvqComposeJob), rec_bytes = (size_t)nlayers * 3u * sizeof(HvqComposeRec);
    std::vector<uint8_t> up(job_bytes + rec_bytes);
    HvqComposeJob *jobs = (HvqComposeJob *)up.data();
    HvqComposeRec *recs = (HvqComposeRec *)(up.data() + job_bytes);
    for (int l = 0; l < nlayers; ++l) {
        const uint8_t *a = nullptr;
        { int rc = picture_source(c, l, streams, ordinals, src, &a); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[l]];
        const HvqComposeLayer &L = layers[l];
        const int sx = L.sx, sy = L.sy, w = L.w ? L.w : s.w, h = L.w ? L.h : s.h;
        if (sx > s.w - w || sy > s.h - h || w > s.w || h > s.h)
            return fail(HVQ_E_ARG, "layer %d: the rectangle %d, %d, %d x %d leaves the %d x %d source", l, sx, sy, w, h, s.w, s.h);
        if (((sx | w | L.dx) & ((1 << s.wshift) - 1)) || ((sy | h | L.dy) & ((1 << s.hshift) - 1)))
            return fail(HVQ_E_ARG, "layer %d: %d, %d, %d x %d -> %d, %d does not lie on the chroma samples of stream %d", l, sx, sy, w, h, L.dx, L.dy, streams[l]);
        plane_walk(slot_shape(s), [&](int p, size_t off, uint32_t nx, uint32_t ny) {
            const int xs = p ? s.wshift : 0, ys = p ? s.hshift : 0;
            recs[(size_t)l * 3u + (size_t)p] = hvq_cp_rec((uint64_t)(uintptr_t)(a + off), nx, ny, sx >> xs, sy >> ys, w >> xs, h >> ys, L.dx >> xs, L.dy >> ys,
                                                          L.weight[p], (uint32_t)L.mode, c->cp_force_general);
            return 0;
        });
    }
    uint32_t max_tiles = 0;
    for (int t = 0; t < ntargets; ++t) {
        const HvqComposeDst &d = dst[t];
        const int dws = d.h_samp == 2, dhs = d.v_samp == 2;
        int64_t gain[3] = { 0, 0, 0 };
        for (int l = d.first; l < d.first + d.count; ++l) {
            const Stream &s = c->streams[(size_t)streams[l]];
            const HvqComposeLayer &L = layers[l];
            if (s.wshift != dws || s.hshift != dhs)
                return fail(HVQ_E_ARG, "target %d, layer %d: stream %d has not the target's sampling %d x %d (scale it first)", t, l, streams[l], d.h_samp, d.v_samp);
            const int w = L.w ? L.w : s.w, h = L.w ? L.h : s.h;
            if (L.dx > d.width - w || L.dy > d.height - h || w > d.width || h > d.height)
                return fail(HVQ_E_ARG, "target %d, layer %d: %d x %d at %d, %d leaves the %d x %d target", t, l, w, h, L.dx, L.dy, d.width, d.height);
            for (int p = 0; p < 3; ++p) gain[p] += L.weight[p] < 0 ? -(int64_t)L.weight[p] : L.weight[p];
        }
        for (int p = 0; p < 3; ++p)
            if (gain[p] > HVQ_CMP_MAX_GAIN) return fail(HVQ_E_ARG, "target %d, plane %d: a gain of %lld (at most %d)", t, p, (long long)gain[p], HVQ_CMP_MAX_GAIN);
        max_tiles = std::max(max_tiles, (uint32_t)plane_walk(slot_shape(d.width, d.height, d.h_samp, d.v_samp), [&](int p, size_t off, uint32_t mx, uint32_t my) {
            HvqComposeJob &j = jobs[(size_t)t * 3u + (size_t)p];
            j = hvq_cp_job((uint64_t)(uintptr_t)((uint8_t *)d.ptr + off), mx, my, (uint32_t)d.first, (uint32_t)d.count, d.shift, d.bias[p], (uint32_t)p);
            return j.tiles;
        }));
    }
    return slot_enqueue(c, hvq_launch_compose, "compose", "hvq_compose.hip", up, ntargets, max_tiles, hip_stream);
}

/* zlib's crc32_combine and adler32_combine (include/hvqm4_amd.h): host only */
HVQ_EXPORT uint32_t hvq_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return hvq_crc32_combine_x(crc_a, crc_b, hvq_gf_xpow8(len_b)); }
HVQ_EXPORT uint32_t hvq_adler32_combine(uint32_t a, uint32_t b, uint64_t len_b) { return hvq_adler32_combine_u(a, b, len_b); }

/* hvq_export_tensors' checks of one destination, for hvq_export_resampled: output size, crop, pitches, alignment (es = element size).
 * The crop and the pitches in effect come back in *g; `bits` = pointer | pitches, for the alignment of the 16-byte stores. */
struct TensorGeom { int x0, y0, cw, ch; int64_t rp, pp; uint64_t bits; };
static int tensor_dst_check(const Stream &s, const HvqTensorDst &d, int i, int64_t es, TensorGeom *g)
{
    if (!d.ptr) return fail(HVQ_E_ARG, "null destination %d", i);
    if (d.out_w < 1 || d.out_h < 1 || d.out_w > 16384 || d.out_h > 16384)
        return fail(HVQ_E_ARG, "destination %d: output size %d x %d outside [1, 16384]", i, d.out_w, d.out_h);
    int x0 = 0, y0 = 0, cw = s.w, ch = s.h;
    if (d.crop_w) { x0 = d.crop_x; y0 = d.crop_y; cw = d.crop_w; ch = d.crop_h; }
    else if (d.crop_x || d.crop_y || d.crop_h) return fail(HVQ_E_ARG, "destination %d: crop_w == 0 takes the whole picture, the other crop fields must be 0", i);
    if (x0 < 0 || y0 < 0 || cw < 1 || ch < 1 || (int64_t)x0 + cw > s.w || (int64_t)y0 + ch > s.h)
        return fail(HVQ_E_ARG, "destination %d: crop (%d, %d, %d, %d) is empty or leaves the %d x %d picture", i, x0, y0, cw, ch, s.w, s.h);
    const int64_t dense = (int64_t)d.out_w * es;
    const int64_t rp = d.row_pitch ? d.row_pitch : dense;
    const int64_t pp = d.plane_pitch ? d.plane_pitch : rp * d.out_h;
    if (rp < dense || rp > ((int64_t)1 << 40) || d.plane_pitch > ((int64_t)1 << 48))
        return fail(HVQ_E_ARG, "destination %d: row pitch %lld outside [%lld, 2^40] or plane pitch above 2^48", i, (long long)rp, (long long)dense);
    if (pp < rp * d.out_h)
        return fail(HVQ_E_ARG, "destination %d: plane pitch %lld below row pitch x height %lld (planes overlap)", i, (long long)pp, (long long)(rp * d.out_h));
    const uint64_t bits = (uint64_t)(uintptr_t)d.ptr | (uint64_t)rp | (uint64_t)pp;
    if (bits & (uint64_t)(es - 1))
        return fail(HVQ_E_ARG, "destination %d: pointer, row pitch and plane pitch must be multiples of the element size %d", i, (int)es);
    *g = TensorGeom{ x0, y0, cw, ch, rp, pp, bits };
    return HVQ_OK;
}

HVQ_EXPORT int hvq_export_tensors(HvqContext *c, int n, const int *streams, const int *ordinals, int dtype,
                                  const float mul[3], const float add[3], const HvqTensorDst *dst, void *hip_stream)
{
    static_assert(sizeof(HvqTensorJob) % 16 == 0, "job tables are uploaded in 16-byte units");
    if (!c || n < 0 || !mul || !add || (n && (!streams || !ordinals || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    if (dtype != HVQ_T_F32 && dtype != HVQ_T_F16 && dtype != HVQ_T_BF16) return fail(HVQ_E_ARG, "bad dtype %d", dtype);
    HvqTensorNorm nm;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(mul[k]) || !std::isfinite(add[k])) return fail(HVQ_E_ARG, "mul / add of channel %d is not finite", k);
        nm.mul[k] = mul[k]; nm.add[k] = add[k];
    }
    if (!n) return HVQ_OK;
    { int rc = chain_begin(c, n, streams, ordinals, nullptr, nullptr); if (rc) return rc; }
    const int64_t es = dtype == HVQ_T_F32 ? 4 : 2;
    const int run = (int)(16 / es);                          /* output samples of a row per lane */
    std::vector<HvqTensorJob> jobs((size_t)n);
    int max_lanes = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *src = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, nullptr, &src); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        const HvqTensorDst &d = dst[i];
        if (!d.ptr) return fail(HVQ_E_ARG, "null destination %d", i);
        if (d.out_w < 1 || d.out_h < 1 || d.out_w > 16384 || d.out_h > 16384)
            return fail(HVQ_E_ARG, "destination %d: output size %d x %d outside [1, 16384]", i, d.out_w, d.out_h);
        int x0 = 0, y0 = 0, cw = s.w, ch = s.h;
        if (d.crop_w) { x0 = d.crop_x; y0 = d.crop_y; cw = d.crop_w; ch = d.crop_h; }
        else if (d.crop_x || d.crop_y || d.crop_h) return fail(HVQ_E_ARG, "destination %d: crop_w == 0 takes the whole picture, the other crop fields must be 0", i);
        if (x0 < 0 || y0 < 0 || cw < 1 || ch < 1 || (int64_t)x0 + cw > s.w || (int64_t)y0 + ch > s.h)
            return fail(HVQ_E_ARG, "destination %d: crop (%d, %d, %d, %d) is empty or leaves the %d x %d picture", i, x0, y0, cw, ch, s.w, s.h);
        const int64_t dense = (int64_t)d.out_w * es;
        const int64_t rp = d.row_pitch ? d.row_pitch : dense;
        const int64_t pp = d.plane_pitch ? d.plane_pitch : rp * d.out_h;
        if (rp < dense || rp > ((int64_t)1 << 40) || d.plane_pitch > ((int64_t)1 << 48))
            return fail(HVQ_E_ARG, "destination %d: row pitch %lld outside [%lld, 2^40] or plane pitch above 2^48", i, (long long)rp, (long long)dense);
        if (pp < rp * d.out_h)
            return fail(HVQ_E_ARG, "destination %d: plane pitch %lld below row pitch x height %lld (planes overlap)", i, (long long)pp, (long long)(rp * d.out_h));
        const uint64_t bits = (uint64_t)(uintptr_t)d.ptr | (uint64_t)rp | (uint64_t)pp;
        if (bits & (uint64_t)(es - 1))
            return fail(HVQ_E_ARG, "destination %d: pointer, row pitch and plane pitch must be multiples of the element size %d", i, (int)es);
        const size_t ny = (size_t)s.w * s.h, nc = (size_t)(s.w >> s.wshift) * (size_t)(s.h >> s.hshift);
        HvqTensorJob &j = jobs[(size_t)i];
        memset(&j, 0, sizeof j);
        j.y = src; j.u = src + ny; j.v = src + ny + nc;
        j.dst = (uint8_t *)d.ptr; j.row_pitch = rp; j.plane_pitch = pp;
        j.w = s.w; j.h = s.h; j.wshift = s.wshift; j.hshift = s.hshift;
        j.x0 = x0; j.y0 = y0; j.cw = cw; j.ch = ch; j.out_w = d.out_w; j.out_h = d.out_h;
        j.sx = (float)cw / (float)d.out_w;                   /* divided here: the device divides nothing */
        j.sy = (float)ch / (float)d.out_h;
        if (!(bits & 15u) && d.out_w % run == 0) {
            j.flags |= HVQ_TJ_VEC;
            if (d.out_w == cw && d.out_h == ch && x0 % run == 0 && s.w % run == 0) j.flags |= HVQ_TJ_IDENT;
        }
        max_lanes = std::max(max_lanes, (d.out_w + run - 1) / run * d.out_h);
    }
    return export_enqueue(c, jobs.data(), (size_t)n * sizeof(HvqTensorJob), hip_stream,
                          [=](const void *tab, hipStream_t st) { return hvq_launch_tensor(tab, n, max_lanes, dtype, &nm, st); });
}

/* ---- the triangle filter's weight tables (include/hvqm4_amd.h: the specification).  Double arithmetic, one rounding per operation:
 * contraction is off in these functions, so that the table is numpy's bit for bit on any host. ---- */
struct ResampleSpan { int first, count; };
static ResampleSpan resample_span(int n_src, int n_out, int j, double *scale_out, double *support_out, double *c_out)
{
#pragma clang fp contract(off)
    const double scale = (double)n_src / (double)n_out;
    const double support = scale > 1.0 ? scale : 1.0;
    const double c = scale * ((double)j + 0.5);
    const int first = std::max((int)(c - support + 0.5), 0);
    const int end = std::min((int)(c + support + 0.5), n_src);
    if (scale_out) { *scale_out = scale; *support_out = support; *c_out = c; }
    return ResampleSpan{ first, end - first };
}

static bool resample_sizes_ok(int n_src, int n_out) { return n_src >= 1 && n_src <= 65535 && n_out >= 1 && n_out <= 16384; }

static size_t resample_weights_len(int n_src, int n_out)
{
    size_t total = 0;
    for (int j = 0; j < n_out; ++j) total += (size_t)resample_span(n_src, n_out, j, nullptr, nullptr, nullptr).count;
    return total;
}

/* first[n_out], count[n_out], weights[resample_weights_len] */
static void resample_fill(int n_src, int n_out, int32_t *first, int32_t *count, float *weights)
{
#pragma clang fp contract(off)
    std::vector<double> u;
    size_t at = 0;
    for (int j = 0; j < n_out; ++j) {
        double scale, support, c;
        const ResampleSpan sp = resample_span(n_src, n_out, j, &scale, &support, &c);
        u.resize((size_t)sp.count);
        double t = 0.0;
        for (int k = 0; k < sp.count; ++k) {
            const double d = ((double)(k + sp.first) - c + 0.5) / support;
            const double v = 1.0 - std::fabs(d);
            u[(size_t)k] = v > 0.0 ? v : 0.0;
            t = k ? t + u[(size_t)k] : u[0];
        }
        for (int k = 0; k < sp.count; ++k) weights[at + (size_t)k] = (float)(u[(size_t)k] / t);
        first[j] = sp.first;
        count[j] = sp.count;
        at += (size_t)sp.count;
    }
}

HVQ_EXPORT int hvq_resample_table(int n_src, int n_out, int32_t *first, int32_t *count, float *weights, size_t weights_cap, size_t *weights_len)
{
    if (!resample_sizes_ok(n_src, n_out)) return fail(HVQ_E_ARG, "n_src %d outside [1, 65535] or n_out %d outside [1, 16384]", n_src, n_out);
    const size_t need = resample_weights_len(n_src, n_out);
    if (weights_len) *weights_len = need;
    if (!weights) return weights_len ? HVQ_OK : fail(HVQ_E_ARG, "a length query needs weights_len");
    if (!first || !count) return fail(HVQ_E_ARG, "bad arguments");
    if (weights_cap < need) return fail(HVQ_E_OVERFLOW, "the table holds %zu weights, room for %zu", need, weights_cap);
    resample_fill(n_src, n_out, first, count, weights);
    return HVQ_OK;
}

/* Output rows of a tile when the tiled body of hvq_yuv_resample_kernel takes a job (16, or 8), 0 when the direct body does: tiled for a
 * downscale along either axis whose largest vertical tile footprint fits HVQ_RS_ROWS source rows.  first and end are monotonic in the
 * output index, so a tile's footprint is [first of its first row, end of its last). */
static int resample_tile_rows(int cw, int ch, int out_w, int out_h, const int32_t *yfirst, const int32_t *ycount)
{
    if (out_w >= cw && out_h >= ch) return 0;
    for (int th : { 16, 8 }) {
        int worst = 0;
        for (int i0 = 0; i0 < out_h; i0 += th) {
            const int i1 = std::min(i0 + th, out_h) - 1;
            worst = std::max(worst, yfirst[i1] + ycount[i1] - yfirst[i0]);
        }
        if (worst <= HVQ_RS_ROWS) return th;
    }
    return 0;
}

HVQ_EXPORT int hvq_resample_tile_rows(int crop_w, int crop_h, int out_w, int out_h)
{
    if (!resample_sizes_ok(crop_w, out_w) || !resample_sizes_ok(crop_h, out_h)) return fail(HVQ_E_ARG, "crop or output size out of range");
    std::vector<int32_t> first((size_t)out_h), count((size_t)out_h);
    for (int i = 0; i < out_h; ++i) {
        const ResampleSpan sp = resample_span(crop_h, out_h, i, nullptr, nullptr, nullptr);
        first[(size_t)i] = sp.first; count[(size_t)i] = sp.count;
    }
    return resample_tile_rows(crop_w, crop_h, out_w, out_h, first.data(), count.data());
}

HVQ_EXPORT int hvq_export_resampled(HvqContext *c, int n, const int *streams, const int *ordinals, int dtype, int filter,
                                    const float mul[3], const float add[3], const HvqTensorDst *dst, void *hip_stream)
{
    if (filter == HVQ_FILTER_BILINEAR) return hvq_export_tensors(c, n, streams, ordinals, dtype, mul, add, dst, hip_stream);
    if (filter != HVQ_FILTER_TRIANGLE && filter != HVQ_FILTER_TRIANGLE_DIRECT) return fail(HVQ_E_ARG, "bad filter %d", filter);
    if (!c || n < 0 || !mul || !add || (n && (!streams || !ordinals || !dst))) return fail(HVQ_E_ARG, "bad arguments");
    if (dtype != HVQ_T_F32 && dtype != HVQ_T_F16 && dtype != HVQ_T_BF16) return fail(HVQ_E_ARG, "bad dtype %d", dtype);
    HvqTensorNorm nm;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(mul[k]) || !std::isfinite(add[k])) return fail(HVQ_E_ARG, "mul / add of channel %d is not finite", k);
        nm.mul[k] = mul[k]; nm.add[k] = add[k];
    }
    if (!n) return HVQ_OK;
    { int rc = chain_begin(c, n, streams, ordinals, nullptr, nullptr); if (rc) return rc; }
    const int64_t es = dtype == HVQ_T_F32 ? 4 : 2;
    const int run = (int)(16 / es);
    /* the upload: n job records, then every distinct (n_src, n_out) axis table once -- first[n_out], start[n_out + 1], weights, padded to
     * 16 bytes; the records carry byte offsets from the end of the records */
    struct AxisTab { int n_src, n_out; uint32_t off; std::vector<int32_t> first, count; };
    std::vector<AxisTab> tabs;
    std::vector<uint8_t> up((size_t)n * sizeof(HvqResampleJob));
    auto axis = [&](int n_src, int n_out) -> int {
        for (size_t t = 0; t < tabs.size(); ++t) if (tabs[t].n_src == n_src && tabs[t].n_out == n_out) return (int)t;
        AxisTab T;
        T.n_src = n_src; T.n_out = n_out;
        T.first.resize((size_t)n_out); T.count.resize((size_t)n_out);
        const size_t nw = resample_weights_len(n_src, n_out);
        const size_t at = up.size(), words = 2u * (size_t)n_out + 1u + nw, bytes = align_up(words * 4u, 16);
        if (at - (size_t)n * sizeof(HvqResampleJob) + bytes > ((size_t)1 << 31)) return -1;
        up.resize(at + bytes);                               /* zero-filled, the padding included */
        std::vector<float> w(nw);
        resample_fill(n_src, n_out, T.first.data(), T.count.data(), w.data());
        int32_t *p = (int32_t *)(up.data() + at);
        memcpy(p, T.first.data(), (size_t)n_out * 4u);
        int32_t sum = 0;
        for (int j = 0; j < n_out; ++j) { p[n_out + j] = sum; sum += T.count[(size_t)j]; }
        p[2 * n_out] = sum;
        memcpy(p + 2 * n_out + 1, w.data(), nw * 4u);
        T.off = (uint32_t)(at - (size_t)n * sizeof(HvqResampleJob));
        tabs.push_back(std::move(T));
        return (int)tabs.size() - 1;
    };
    int max_wgs = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t *src = nullptr;
        { int rc = picture_source(c, i, streams, ordinals, nullptr, &src); if (rc) return rc; }
        const Stream &s = c->streams[(size_t)streams[i]];
        const HvqTensorDst &d = dst[i];
        TensorGeom g;
        { int rc = tensor_dst_check(s, d, i, es, &g); if (rc) return rc; }
        const int tx = axis(g.cw, d.out_w), ty = tx < 0 ? -1 : axis(g.ch, d.out_h);
        if (tx < 0 || ty < 0) return fail(HVQ_E_OVERFLOW, "the weight tables of the call exceed 2 GiB");
        const size_t ny = (size_t)s.w * s.h, nc = (size_t)(s.w >> s.wshift) * (size_t)(s.h >> s.hshift);
        HvqResampleJob j;
        memset(&j, 0, sizeof j);
        j.y = src; j.u = src + ny; j.v = src + ny + nc;
        j.dst = (uint8_t *)d.ptr; j.row_pitch = g.rp; j.plane_pitch = g.pp;
        j.w = s.w; j.wshift = s.wshift; j.hshift = s.hshift;
        j.x0 = g.x0; j.y0 = g.y0; j.out_w = d.out_w; j.out_h = d.out_h;
        j.xtab = tabs[(size_t)tx].off; j.ytab = tabs[(size_t)ty].off;
        if (!(g.bits & 15u) && d.out_w % run == 0) j.flags |= HVQ_RJ_VEC;
        const int th = filter == HVQ_FILTER_TRIANGLE_DIRECT ? 0
                     : resample_tile_rows(g.cw, g.ch, d.out_w, d.out_h, tabs[(size_t)ty].first.data(), tabs[(size_t)ty].count.data());
        int wgs;
        if (th) {
            j.flags |= HVQ_RJ_TILED;
            j.tile_h = th;
            j.tiles_x = (uint32_t)((d.out_w + HVQ_RS_TILE_W - 1) / HVQ_RS_TILE_W);
            wgs = (int)j.tiles_x * ((d.out_h + th - 1) / th);
        } else {
            wgs = ((d.out_w + run - 1) / run * d.out_h + 255) / 256;
        }
        memcpy(up.data() + (size_t)i * sizeof(HvqResampleJob), &j, sizeof j);
        max_wgs = std::max(max_wgs, wgs);
    }
    return export_enqueue(c, up.data(), up.size(), hip_stream,
                          [=](const void *tab, hipStream_t st) { return hvq_launch_resample(tab, n, max_wgs, dtype, &nm, st); });
}

HVQ_EXPORT int hvq_rgb_bench(HvqContext *c, int reps, float *gpu_ms, uint64_t *bytes_per_rep, uint32_t *pictures)
{
    if (!c || reps < 1) return fail(HVQ_E_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    { int rc = flush_end(c); if (rc) return rc; }
    std::vector<HvqRgbJob> jobs;
    uint64_t bytes = 0;
    for (auto &s : c->streams) {
        if (!s.open || s.npics == 0 || s.pic_bytes != (uint32_t)(s.w * s.h * 3 / 2)) continue;
        int slot = s.pic_slot[(size_t)s.npics - 1];
        if (slot < 0) continue;
        jobs.push_back(rgb420_job(s.slot_ptr(slot), s.w, s.h));
        bytes += (uint64_t)s.w * s.h * 9 / 2;              /* 1.5 B/px read + 3 B/px written */
    }
    if (jobs.empty()) return fail(HVQ_E_STATE, "no resident 4:2:0 picture");
    int rc = rgb_run(c, jobs.data(), (int)jobs.size(), reps, gpu_ms);
    if (rc) return rc;
    if (bytes_per_rep) *bytes_per_rep = bytes;
    if (pictures) *pictures = (uint32_t)jobs.size();
    return HVQ_OK;
}

/* Measurement helper: `reps` pinned-host -> device copies of `bytes` on the context's copy stream, timed with HIP events: the PCIe
 * rate a batch's bitstream upload can reach on this box (the bound of streaming from host memory, whatever the kernels do). */
HVQ_EXPORT int hvq_h2d_probe(HvqContext *c, size_t bytes, int reps, double *gb_per_s)
{
    if (!c || !bytes || reps < 1 || !gb_per_s) return fail(HVQ_E_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    void *h = nullptr, *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&d, bytes);
    if (e == hipSuccess) { memset(h, 0x5a, bytes); e = hipEventCreate(&e0); }
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->copy_stream);   /* warm-up: mappings, clocks */
    if (e == hipSuccess) e = hipEventRecord(e0, c->copy_stream);
    for (int r = 0; r < reps && e == hipSuccess; ++r) e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(e1, c->copy_stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    HIPCHK(e);
    *gb_per_s = ms > 0 ? (double)bytes * reps / (ms * 1e-3) / 1e9 : 0.0;
    return HVQ_OK;
}

/* self-test: out[0..15] = the kernels' divTable quotients 256 / d, out[16..271] = their mcdivTable quotients 4096 / d (h4m:265-273) */
HVQ_EXPORT int hvq_debug_table_divisions(HvqContext *c, uint32_t *out)
{
    if (!c || !out) return fail(HVQ_E_ARG, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    uint32_t *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, 272 * sizeof(uint32_t)));
    hipError_t e = hvq_launch_table_div(d, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d, 272 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(e);
    return HVQ_OK;
}

HVQ_EXPORT int hvq_get_stats(HvqContext *c, HvqStats *out)
{
    if (!c || !out) return fail(HVQ_E_ARG, "bad arguments");
    { int rc = flush_end(c); if (rc) return rc; }
    *out = c->stats;
    out->parse_seconds = c->parse_seconds;
    out->copy_bytes = c->copy_bytes.load(); out->copy_seconds = (double)c->copy_ns.load() * 1e-9;
    return HVQ_OK;
}

/* ------------------------------------------------------------------ SDK entry points */
namespace {

constexpr uint64_t SDK_MAGIC = 0x4856514d34414d44ull;   /* "HVQM4AMD" */

struct SdkBinding {
    std::mutex mu;                     /* one decode at a time per SeqObj; different SeqObjs decode concurrently (each has its own context) */
    HvqContext *ctx = nullptr;
    int stream = -1;
    int w = 0, h = 0, hs = 0, vs = 0, is15 = -1;
    uint32_t pic_bytes = 0;
    uint32_t max_frame = 0;            /* HVQM4SetMaxFrameSize: readable bytes at `frame` (0 = unknown) */
    /* what the three device slots hold: the host buffer whose content was last written there by this library */
    const void *host[3] = { nullptr, nullptr, nullptr };
    bool valid[3] = { false, false, false };
    /* pinned staging, one picture each: [0], [1] reference pictures on their way up (their DMA runs beside the host parse),
     * [2] the decoded picture on its way down (one DMA, then one memcpy into the caller's pageable buffer) */
    uint8_t *stage[3] = { nullptr, nullptr, nullptr };
};

struct SdkHeader {          /* lives at the start of the caller's work buffer */
    uint64_t magic;
    SdkBinding *binding;
};

std::mutex g_sdk_mu;                    /* the registry of bindings */
std::mutex g_sdk_ctx_mu;                /* the probe context (its own lock: it is taken by a decode that holds its binding's lock) */
HvqContext *g_sdk_ctx = nullptr;
std::set<SdkBinding *> g_bindings;

void sdk_fail(int code)
{
    g_sdk_err = code;
    fprintf(stderr, "hvqm4_amd: %s\n", g_err.c_str());
}

int sdk_device()
{
    const char *dev = getenv("HVQM4_AMD_DEVICE");
    return dev ? atoi(dev) : 0;
}

HvqContext *sdk_context()              /* HVQM4InitDecoder: a missing GPU is reported at init time */
{
    if (g_sdk_ctx) return g_sdk_ctx;
    int rc = hvq_context_create(sdk_device(), &g_sdk_ctx);
    if (rc) { sdk_fail(rc); g_sdk_ctx = nullptr; }
    return g_sdk_ctx;
}

void sdk_free_binding(SdkBinding *b)
{
    if (b->ctx) {
        (void)hipSetDevice(b->ctx->device);
        (void)hvq_sync(b->ctx);
        for (auto &p : b->stage) if (p) { (void)hipHostFree(p); p = nullptr; }
        hvq_context_destroy(b->ctx);            /* closes its stream */
    }
    delete b;
}

void sdk_release_locked(SdkHeader *hd)
{
    if (hd->magic == SDK_MAGIC && g_bindings.count(hd->binding)) {
        SdkBinding *b = hd->binding;
        g_bindings.erase(b);
        { std::lock_guard<std::mutex> lk(b->mu); }      /* a decode in flight on another thread ends first */
        sdk_free_binding(b);
    }
    hd->magic = 0; hd->binding = nullptr;
}

/* The SeqObj's binding with ITS lock held, or an unlocked lock + error.  The binding's lock is taken while the registry lock is still
 * held (hand-over): a HVQM4SetBuffer / HVQM4ReleaseBuffer of the same SeqObj on another thread can then no longer free the binding
 * between the look-up and the decode's own lock (advisor finding of round 4: it could).  try_lock + retry, so that a second thread
 * decoding on the SAME SeqObj (it waits) never blocks the registry for the players of other SeqObjs; nothing that holds a binding's
 * lock waits for the registry lock (the probe context has a lock of its own), so the order registry -> binding cannot deadlock. */
std::unique_lock<std::mutex> sdk_lookup(SeqObj *seq, SdkBinding **out)
{
    *out = nullptr;
    for (;;) {
        {
            std::lock_guard<std::mutex> lk(g_sdk_mu);
            if (!seq || !seq->state) { fail(HVQ_E_ARG, "SeqObj has no work buffer (call HVQM4SetBuffer)"); sdk_fail(HVQ_E_ARG); return {}; }
            SdkHeader *hd = (SdkHeader *)seq->state;
            if (hd->magic != SDK_MAGIC || !g_bindings.count(hd->binding)) { fail(HVQ_E_STATE, "work buffer was not initialised by HVQM4SetBuffer"); sdk_fail(HVQ_E_STATE); return {}; }
            std::unique_lock<std::mutex> bl(hd->binding->mu, std::try_to_lock);
            if (bl.owns_lock()) { *out = hd->binding; return bl; }
        }
        std::this_thread::yield();
    }
}

/* (re)open the device stream when the 1.3/1.5 switch byte changed (h4m:2414-2417); called with the binding's lock held */
bool sdk_open(SdkBinding *b, SeqObj *seq)
{
    const int is15 = seq->state->padding[0] != 0;
    if (b->stream >= 0 && b->is15 != is15) { hvq_stream_close(b->ctx, b->stream); b->stream = -1; }
    if (b->stream < 0) {
        if (!b->ctx) {
            {   /* the context HVQM4InitDecoder probed the device with serves the first SeqObj */
                std::lock_guard<std::mutex> lk(g_sdk_ctx_mu);
                b->ctx = g_sdk_ctx; g_sdk_ctx = nullptr;
            }
            if (!b->ctx) {
                int rc = hvq_context_create(sdk_device(), &b->ctx);
                if (rc) { b->ctx = nullptr; sdk_fail(rc); return false; }
            }
        }
        int sid = hvq_stream_open(b->ctx, b->w, b->h, b->hs, b->vs, is15, 3);
        if (sid < 0) { sdk_fail(sid); return false; }
        b->stream = sid; b->is15 = is15;
        b->pic_bytes = hvq_stream_pic_bytes(b->ctx, sid);
        {   /* One synchronous picture at a time: its sections are parsed side by side by a small pool of the SeqObj's parser (78 % of a
             * call was the parse on ONE core).  HVQM4_AMD_SDK_PARSE_THREADS (default 4, capped by the cores this process may run on;
             * 1 = the calling thread alone). */
            static const int want = getenv("HVQM4_AMD_SDK_PARSE_THREADS") ? atoi(getenv("HVQM4_AMD_SDK_PARSE_THREADS")) : 4;
            const int cores = (int)std::max(1u, std::thread::hardware_concurrency());
            (void)hvq_parser_set_threads(b->ctx->streams[(size_t)sid].parser, std::max(1, std::min(want, cores)));
        }
        for (auto &p : b->stage)
            if (!p && hipHostMalloc((void **)&p, b->pic_bytes, hipHostMallocDefault) != hipSuccess) p = nullptr;   /* without staging: plain copies */
        for (int i = 0; i < 3; ++i) b->valid[i] = false;
    }
    return true;
}

/* One synchronous picture: upload the caller's reference pictures, reconstruct, read back.  ONE wait on the GPU per call.
 * HVQM4_AMD_TRUST_PICTURES=1: a reference picture is not uploaded again when `past` / `future` is a host buffer this
 * library itself filled last (as `present` of an earlier call on the same SeqObj) and its device copy is still in place --
 * valid for players that do not touch decoded pictures, which the SDK contract does not promise (hence opt-in). */
void sdk_decode(SeqObj *seq, int ftype, const uint8_t *frame, void *present, const void *past, const void *future)
{
    SdkBinding *b = nullptr;
    std::unique_lock<std::mutex> lk = sdk_lookup(seq, &b);
    if (!b) return;
    /* HVQM4_AMD_SDK_TIMING=1: where a call's time goes, on stderr (development aid) */
    static const bool timing = getenv("HVQM4_AMD_SDK_TIMING") != nullptr;
    double tm[6] = { 0, 0, 0, 0, 0, 0 };
    if (timing) tm[0] = now_ms();
    if (!sdk_open(b, seq)) return;
    HvqContext *c = b->ctx;
    Stream &s = c->streams[(size_t)b->stream];
    /* the SDK signatures carry no length: it comes from the picture's own section table (hvq_picture_length), so that the
     * host parser bounds every later read */
    size_t len = 0;
    { int rc = hvq_picture_length(frame, ftype, b->max_frame, &len);
      if (rc) { fail(rc, "malformed picture: a section lies outside the frame"); sdk_fail(rc); return; } }
    static const bool trust = getenv("HVQM4_AMD_TRUST_PICTURES") && atoi(getenv("HVQM4_AMD_TRUST_PICTURES")) > 0;
    int used[2] = { -1, -1 };
    /* a call that fails half way leaves uploads in flight and slots half written: nothing on the device is trusted afterwards */
    struct Undo { SdkBinding *b; HvqContext *c; bool ok; ~Undo() { if (!ok) { (void)hipStreamSynchronize(c->stream); for (auto &v : b->valid) v = false; } } } undo{ b, c, false };
    /* device slot that holds `src`: the resident copy if trusted, else a slot not already taken, refreshed from the host.  The
     * upload goes through pinned staging and is asynchronous: it runs while the host parses the picture */
    auto bring = [&](const void *src, int k) -> int {
        int slot = -1;
        if (trust)
            for (int i = 0; i < 3; ++i) if (b->valid[i] && b->host[i] == src && i != used[0]) slot = i;
        if (slot < 0) {
            for (int i = 0; i < 3 && slot < 0; ++i) if (i != used[0] && !(b->valid[i] && trust && (b->host[i] == past || b->host[i] == future))) slot = i;
            if (slot < 0) slot = used[0] == 0 ? 1 : 0;
            const void *from = src;
            if (b->stage[k]) { memcpy(b->stage[k], src, s.pic_bytes); from = b->stage[k]; }
            hipError_t e = hipMemcpyAsync(s.slot_ptr(slot), from, s.pic_bytes, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) { fail(HVQ_E_HIP, "upload of reference picture: %s", hipGetErrorString(e)); sdk_fail(HVQ_E_HIP); return -1; }
            b->host[slot] = src; b->valid[slot] = true;
        }
        used[k] = slot;
        return slot;
    };
    s.anchor_old = -1; s.anchor_new = -1;
    if (ftype == HVQ_FRAME_P) {
        const int ps = bring(past, 0);
        if (ps < 0) return;
        s.anchor_new = ps;                               /* swapped to "past" by the submit's rotation */
    } else if (ftype == HVQ_FRAME_B) {
        const int ps = bring(past, 0);
        if (ps < 0) return;
        const int fs = bring(future, 1);
        if (fs < 0) return;
        s.anchor_old = ps; s.anchor_new = fs;
    }
    int dst = -1;
    for (int i = 0; i < 3; ++i) if (i != used[0] && i != used[1] && (dst < 0 || b->host[i] == present)) dst = i;
    s.ring = dst;                                        /* alloc_slot takes the first slot from here that is no anchor */
    b->valid[dst] = false;
    s.sdk_present = ftype == HVQ_FRAME_P ? present : nullptr;   /* a self-referencing P picture reads the caller's buffer (h4m:2058-2061) */
    if (timing) tm[1] = now_ms();
    int ord = hvq_stream_submit(c, b->stream, ftype, frame, len);
    c->streams[(size_t)b->stream].sdk_present = nullptr;
    if (ord < 0) { sdk_fail(ord); return; }
    if (timing) tm[2] = now_ms();
    int rc = hvq_flush(c);
    if (rc) { sdk_fail(rc); return; }
    if (timing) tm[3] = now_ms();
    if (b->stage[2]) {
        /* the picture's DMA is queued behind its launches: one wait for both, then one memcpy into the caller's buffer */
        const int slot = s.pic_slot[(size_t)ord];
        hipError_t e = slot < 0 ? hipErrorInvalidValue : hipMemcpyAsync(b->stage[2], s.slot_ptr(slot), s.pic_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { fail(HVQ_E_HIP, "download of the decoded picture: %s", hipGetErrorString(e)); sdk_fail(HVQ_E_HIP); return; }
        memcpy(present, b->stage[2], s.pic_bytes);
    } else {
        rc = hvq_read_picture(c, b->stream, ord, present, s.pic_bytes);
        if (rc) { sdk_fail(rc); return; }
    }
    b->host[dst] = present; b->valid[dst] = true;        /* host and device copies are the same now */
    undo.ok = true;
    if (timing) {
        tm[4] = now_ms();
        fprintf(stderr, "sdk_decode 0x%x: bind + reference uploads %.3f | host parse %.3f | flush (uploads, launches) %.3f | wait + download %.3f | total %.3f ms\n",
                ftype, tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], tm[4] - tm[0]);
    }
}

}  // namespace

HVQ_EXPORT void HVQM4InitDecoder(void)
{
    /* the reference fills divTable/mcdivTable here (h4m:265-278); ours are compile-time constants
     * in the kernel.  Probe the device early so a missing GPU is reported at init time. */
    std::lock_guard<std::mutex> lk(g_sdk_ctx_mu);
    (void)sdk_context();
}

HVQ_EXPORT void HVQM4InitSeqObj(SeqObj *seqobj, VideoInfo *videoinfo)
{
    seqobj->width = videoinfo->hres;
    seqobj->height = videoinfo->vres;
    seqobj->h_samp = videoinfo->h_samp;
    seqobj->v_samp = videoinfo->v_samp;
}

HVQ_EXPORT uint32_t HVQM4BuffSize(SeqObj *seqobj)
{
    /* same arithmetic as h4m:828-840 so callers allocate what they always did */
    uint32_t hb = seqobj->width / 4, vb = seqobj->height / 4;
    uint32_t yb = (hb + 2) * (vb + 2);
    uint32_t uhb = seqobj->h_samp == 2 ? hb / 2 : hb, uvb = seqobj->v_samp == 2 ? vb / 2 : vb;
    uint32_t uvblocks = (uhb + 2) * (uvb + 2);
    return (uint32_t)sizeof(VideoState) + (yb + uvblocks * 2) * (uint32_t)sizeof(uint16_t);
}

HVQ_EXPORT void HVQM4SetBuffer(SeqObj *seqobj, void *workbuff)
{
    std::lock_guard<std::mutex> lk(g_sdk_mu);
    SdkHeader *hd = (SdkHeader *)workbuff;
    sdk_release_locked(hd);                 /* re-binding an already bound buffer must not leak */
    seqobj->state = (VideoState *)workbuff;
    SdkBinding *b = new SdkBinding();
    b->w = seqobj->width; b->h = seqobj->height; b->hs = seqobj->h_samp; b->vs = seqobj->v_samp;
    g_bindings.insert(b);
    hd->magic = SDK_MAGIC;
    hd->binding = b;
}

HVQ_EXPORT void HVQM4ReleaseBuffer(SeqObj *seqobj)
{
    std::lock_guard<std::mutex> lk(g_sdk_mu);
    if (seqobj && seqobj->state) sdk_release_locked((SdkHeader *)seqobj->state);
}

HVQ_EXPORT void HVQM4SetMaxFrameSize(SeqObj *seqobj, uint32_t bytes)
{
    std::lock_guard<std::mutex> lk(g_sdk_mu);
    if (!seqobj || !seqobj->state) return;
    SdkHeader *hd = (SdkHeader *)seqobj->state;
    if (hd->magic == SDK_MAGIC && g_bindings.count(hd->binding)) hd->binding->max_frame = bytes;
}

HVQ_EXPORT void HVQM4SetVersion15(SeqObj *seqobj, int is15)
{
    if (seqobj && seqobj->state) seqobj->state->padding[0] = is15 ? 1 : 0;
}

HVQ_EXPORT void HVQM4DecodeIpic(SeqObj *seqobj, uint8_t const *frame, void *present)
{
    sdk_decode(seqobj, HVQ_FRAME_I, frame, present, nullptr, nullptr);
}

HVQ_EXPORT void HVQM4DecodePpic(SeqObj *seqobj, uint8_t const *frame, void *present, void *past)
{
    sdk_decode(seqobj, HVQ_FRAME_P, frame, present, past, nullptr);
}

HVQ_EXPORT void HVQM4DecodeBpic(SeqObj *seqobj, uint8_t const *frame, void *present, void *past, void *future)
{
    sdk_decode(seqobj, HVQ_FRAME_B, frame, present, past, future);
}

HVQ_EXPORT int HVQM4GetLastError(void)
{
    int e = g_sdk_err;
    g_sdk_err = 0;
    return e;
}

HVQ_EXPORT const char *HVQM4GetLastErrorString(void) { return g_err.c_str(); }
