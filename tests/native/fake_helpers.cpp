/*
 * tests/native/fake_helpers.cpp -- TEST INFRASTRUCTURE: the LDS, occupancy and scratch sizing helpers that hvqm4_amd/csrc/hvq_runtime.cpp
 * imports from the HIP units (hvq_kernels.hip, hvq_gparse.hip), restated for the CPU fake device.  A unit of its own, so that
 * tests/test_fake_device.py can load it beside the real library and compare the two over the whole grid of shapes.
 */
#include <algorithm>
#include <cstdint>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_gparse_core.h"

static const uint32_t INL_NEST_LDS = (HVQ_NESTP_BYTES + 8 + 15) / 16 * 16;       /* HVQ_INL_NEST_LDS */

extern "C" uint32_t hvq_recon_inline_static_lds(uint32_t, uint32_t items_cap)
{
    return INL_NEST_LDS + 4u * (16u + 4u + 3u) * items_cap + 16u;                /* hvq_inl_static_lds: accumulators, block, records; counter */
}

extern "C" uint32_t hvq_recon_inline_dyn_lds(uint32_t pair_cap, uint32_t pool_cap)
{
    return 4u * (((std::max(pair_cap, 1u) + 3u) & ~3u) + ((pool_cap + 3u) & ~3u));
}

extern "C" uint32_t hvq_recon_inline_max_wgs(uint32_t tiles_per_wg, uint32_t items_cap)
{
    return tiles_per_wg >= 2 && std::min(items_cap, 512u) >= 128u ? 7u : 8u;     /* hvq_inl_waves: HVQ_SEVEN_WG_CAP, HVQ_MIN_WAVES */
}

extern "C" uint32_t hvq_gparse_scratch_bytes(uint32_t total_blocks, uint32_t total_runs, uint32_t nmb) { return gp_scratch_bytes(total_blocks, total_runs, nmb); }

/* the real one asks the HIP runtime (it needs a device); the parse kernel is built for eight workgroups per CU.  Diagnostics only. */
extern "C" int hvq_parse_occupancy(uint32_t) { return 8; }
