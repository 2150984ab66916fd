/*
 * tests/native/fake_driver_common.h -- TEST INFRASTRUCTURE: what the stand-alone fake-device drivers (fake_driver.cpp and the
 * fake_*_driver.cpp of the export-chain calls) have in common: the clips of the golden directory with their pictures, a stream that
 * holds a decoded clip, the caller's stream, CRC-32, and the two macros that end the program when a call of the library or of the fake
 * HIP fails.  Only what is the same in every driver is here; a driver says who it is before it includes the header:
 *
 *   #define DRIVER_NAME "fake_metrics_driver"
 *   #include "fake_driver_common.h"
 *
 * and sets g_golden, g_out and g_res from its arguments in main.
 */
#ifndef FAKE_DRIVER_COMMON_H
#define FAKE_DRIVER_COMMON_H

#ifndef DRIVER_NAME
#error "a driver defines DRIVER_NAME (the program's name in its messages) before it includes fake_driver_common.h"
#endif

#include "fake_device.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/hvqm4_amd.h"

struct Pic { int type; const uint8_t *p; size_t len; };
struct Clip {
    std::string name;
    std::vector<uint8_t> data;
    HvqH4mInfo info;
    std::vector<Pic> pics;
};

static std::string g_golden, g_out;
static FILE *g_res;
static std::map<std::string, Clip> g_clips;

#define CHECK(expr) do { const int rc_ = (int)(expr); if (rc_ < 0) { fprintf(stderr, DRIVER_NAME ": %s = %d: %s\n", #expr, rc_, hvq_last_error_string()); exit(3); } } while (0)
#define HIP(expr) do { if ((expr) != hipSuccess) { fprintf(stderr, DRIVER_NAME ": %s failed\n", #expr); exit(3); } } while (0)

static const Clip &clip(const std::string &name)
{
    auto it = g_clips.find(name);
    if (it != g_clips.end()) return it->second;
    Clip &c = g_clips[name];
    c.name = name;
    const std::string path = g_golden + "/" + name + ".h4m";
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, DRIVER_NAME ": cannot open %s\n", path.c_str()); exit(2); }
    fseek(f, 0, SEEK_END);
    c.data.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(c.data.data(), 1, c.data.size(), f) != c.data.size()) exit(2);
    fclose(f);
    CHECK(hvq_h4m_header(c.data.data(), c.data.size(), &c.info));
    HvqH4mIter it2;
    hvq_h4m_begin(&it2);
    int type; uint32_t disp; const uint8_t *p; size_t len;
    while (hvq_h4m_next(c.data.data(), c.data.size(), &it2, &type, &disp, &p, &len) == 1) c.pics.push_back(Pic{ type, p, len });
    return c;
}

/* a stream of the clip's geometry with a slot for every picture of the clip and `extra` more */
static inline int open_stream(HvqContext *ctx, const Clip &c, int extra = 3)
{
    const int sid = hvq_stream_open(ctx, c.info.width, c.info.height, c.info.h_samp, c.info.v_samp, c.info.is_1_5, (int)c.pics.size() + extra);
    CHECK(sid);
    return sid;
}

/* ... with the clip decoded into it (host parse, one flush) */
static inline int decode(HvqContext *ctx, const Clip &c, int extra = 3)
{
    const int sid = open_stream(ctx, c, extra);
    for (const Pic &p : c.pics) CHECK(hvq_stream_submit(ctx, sid, p.type, p.p, p.len));
    CHECK(hvq_flush(ctx));
    return sid;
}

static inline hipStream_t caller_stream()
{
    hipStream_t s = nullptr;
    HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}

static inline uint32_t crc32_of(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

#endif
