/*
 * tests/native/fake_driver_common.h -- TEST INFRASTRUCTURE: what the stand-alone fake-device drivers (fake_driver.cpp and the
 * fake_*_driver.cpp of the export-chain calls) have in common: the clips of the golden directory with their pictures, a stream that
 * holds a decoded clip, the caller's stream, CRC-32, the two macros that end the program when a call of the library or of the fake
 * HIP fails, a picture read back (as it is, or inverted) and uploaded as the caller's memory, the frame of a scenario (run_scenario)
 * and the frame of the program (driver_main).  Only what is the same in every driver is here; fake_slot_driver.h and
 * fake_record_driver.h add what the drivers of one family of calls share.  A driver says who it is before it includes a header:
 *
 *   #define DRIVER_NAME "fake_metrics_driver"
 *   #include "fake_record_driver.h"
 *
 * and either hands its scenarios to driver_main or sets g_golden, g_out and g_res from its arguments in a main of its own.
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
#include <initializer_list>
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
static std::vector<std::string> g_extra;             /* what follows the golden directory on the command line (driver_main) */
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

/* picture k of stream sid read back */
static inline std::vector<uint8_t> read_back(HvqContext *ctx, int sid, int k)
{
    std::vector<uint8_t> host(hvq_stream_pic_bytes(ctx, sid));
    CHECK(hvq_read_picture(ctx, sid, k, host.data(), host.size()));
    return host;
}

/* ... with every byte inverted */
static inline std::vector<uint8_t> inverted(HvqContext *ctx, int sid, int k)
{
    std::vector<uint8_t> host = read_back(ctx, sid, k);
    for (uint8_t &x : host) x = (uint8_t)(255 - x);
    return host;
}

/* the caller's memory: `host` in device memory, `offset` bytes into an allocation of its own, which `keep` gets -> where the bytes lie */
static inline void *uploaded(const std::vector<uint8_t> &host, size_t offset, std::vector<void *> *keep)
{
    void *d = nullptr;
    HIP(hipMalloc(&d, host.size() + offset));
    keep->push_back(d);
    HIP(hipMemcpy((uint8_t *)d + offset, host.data(), host.size(), hipMemcpyHostToDevice));
    return (uint8_t *)d + offset;
}

/* The frame of a scenario: a context and the caller's stream around `body`, destroyed in that order.  A body that destroys the context
 * itself, with work still queued, sets `ctx` to null. */
static inline void run_scenario(void (*body)(HvqContext *&ctx, hipStream_t caller))
{
    HvqContext *ctx = nullptr;
    CHECK(hvq_context_create(0, &ctx));
    hipStream_t caller = caller_stream();
    body(ctx, caller);
    if (ctx) hvq_context_destroy(ctx);
    HIP(hipStreamDestroy(caller));
}

/* The frame of the program: <scenario> <outdir> <golden dir> and whatever `more` names (it lands in g_extra); the scenario's body runs
 * inside run_scenario, a `plain` one (host only) as it is; then everything the fake device still holds is drained. */
struct Scenario { const char *name; void (*body)(HvqContext *&ctx, hipStream_t caller); void (*plain)() = nullptr; };

static inline int driver_main(int argc, char **argv, std::initializer_list<Scenario> scenarios, const char *more = "")
{
    if (argc < 4) { fprintf(stderr, "usage: " DRIVER_NAME " <scenario> <outdir> <golden dir>%s\n", more); return 2; }
    g_out = argv[2]; g_golden = argv[3];
    g_extra.assign(argv + 4, argv + argc);
    const Scenario *sc = nullptr;
    for (const Scenario &s : scenarios)
        if (!strcmp(s.name, argv[1])) sc = &s;
    if (!sc) { fprintf(stderr, DRIVER_NAME ": unknown scenario %s\n", argv[1]); return 2; }
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, DRIVER_NAME ": cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc->body) run_scenario(sc->body);
    else sc->plain();
    fake_drain_all();
    fclose(g_res);
    return 0;
}

#endif
