/*
 * tests/native/fake_slot_driver.h -- TEST INFRASTRUCTURE: what the drivers of the calls that write uint8 pictures in slot layout
 * (fake_{scale,filter,warp,compose,rank,map}_driver.cpp) have in common on top of fake_driver_common.h: a geometry and its bytes, the
 * fill rules the tests know, the guarded room an output is written into and its read-back, and the picture and the item of a call.
 * A driver defines DRIVER_NAME and includes this header; its own are its input files, its call_* (the library call and its forms), the
 * format of its P line and its scenarios.
 */
#ifndef FAKE_SLOT_DRIVER_H
#define FAKE_SLOT_DRIVER_H

#include "fake_driver_common.h"

struct Geom { int w, h, hs, vs; };

static const size_t GUARD = 256;                     /* bytes around an output that no call may write */
static const uint8_t SENTINEL = 0xA5;                /* ... and what they and the output hold before the call */

static inline Geom geom_of(const Clip &c) { return Geom{ c.info.width, c.info.height, c.info.h_samp, c.info.v_samp }; }
static inline size_t bytes_of(Geom g) { return (size_t)g.w * g.h + 2u * (size_t)(g.w >> (g.hs == 2)) * (size_t)(g.h >> (g.vs == 2)); }

/* A picture of geometry g filled by a rule the tests know: synth (byte i = ((i + k) * 2654435761 mod 2^32) >> 13 & 255), flat (every
 * byte k), check (a 0 / 255 checkerboard, 255 where x + y + k is odd, in every plane) */
static inline std::vector<uint8_t> filled(Geom g, const std::string &form, int k)
{
    const size_t pb = bytes_of(g);
    std::vector<uint8_t> host(pb);
    if (form == "synth") for (size_t i = 0; i < pb; ++i) host[i] = (uint8_t)(((uint32_t)((uint32_t)(i + (size_t)k) * 2654435761u)) >> 13);
    else if (form == "flat") memset(host.data(), k, pb);
    else if (form == "check") {
        size_t at = 0;
        for (int p = 0; p < 3; ++p) {
            const size_t pw = (size_t)(p ? g.w >> (g.hs == 2) : g.w), ph = (size_t)(p ? g.h >> (g.vs == 2) : g.h);
            for (size_t y = 0; y < ph; ++y)
                for (size_t x = 0; x < pw; ++x) host[at++] = (uint8_t)(((x + y + (size_t)k) & 1u) ? 255 : 0);
        }
    } else { fprintf(stderr, DRIVER_NAME ": form %s\n", form.c_str()); exit(2); }
    return host;
}

/* The room of an output of nb bytes: an allocation of its own filled with the sentinel, `front` guard bytes (GUARD, or 0) before the
 * picture and GUARD behind it -> the allocation; the picture lies at + front */
static inline uint8_t *guarded_room(size_t nb, size_t front = GUARD)
{
    void *o = nullptr;
    HIP(hipMalloc(&o, front + nb + GUARD));
    std::vector<uint8_t> fill(front + nb + GUARD, SENTINEL);
    HIP(hipMemcpy(o, fill.data(), fill.size(), hipMemcpyHostToDevice));
    return (uint8_t *)o;
}

/* ... read back: the CRC-32 of the picture, and whether the guard bytes still hold the sentinel */
struct ReadBack { uint32_t crc; int guard; };
static inline ReadBack read_room(const uint8_t *room, size_t nb, size_t front = GUARD)
{
    std::vector<uint8_t> host(front + nb + GUARD);
    HIP(hipMemcpy(host.data(), room, host.size(), hipMemcpyDeviceToHost));
    int guard = 1;
    for (size_t g = 0; g < GUARD; ++g) guard &= (g >= front || host[g] == SENTINEL) && host[front + nb + g] == SENTINEL;
    return ReadBack{ crc32_of(host.data() + front, nb), guard };
}

/* One picture of a call and what the test is told about it: (sid, k, src) go to the library, (source, form, kk, g) into the P line */
struct Picture { int sid, k; const void *src; std::string source, form; int kk; Geom g; };

static inline Picture resident_picture(int sid, const Clip &c, int k) { return Picture{ sid, k, nullptr, c.name, "pic", k, geom_of(c) }; }

/* the caller's memory: picture k of stream sid, every byte inverted, `offset` bytes into an allocation */
static inline Picture inverted_picture(HvqContext *ctx, int sid, const Clip &c, int k, size_t offset, std::vector<void *> *keep)
{
    return Picture{ sid, -1, uploaded(inverted(ctx, sid, k), offset, keep), c.name, "inv", k, geom_of(c) };
}

/* the caller's memory filled by a rule; the stream `sid` carries its geometry */
static inline Picture made_picture(int sid, Geom g, const char *form, int k, std::vector<void *> *keep)
{
    return Picture{ sid, -1, uploaded(filled(g, form, k), 0, keep), "synth", form, k, g };
}

/* ... with the one number most calls add per picture: the entry of the call's table (a filter, a rank, a table, a warp) */
struct Item : Picture { int entry; };

static inline Item resident(int sid, const Clip &c, int k, int entry) { return Item{ resident_picture(sid, c, k), entry }; }
static inline Item in_memory(HvqContext *ctx, int sid, const Clip &c, int k, size_t offset, std::vector<void *> *keep, int entry)
{
    return Item{ inverted_picture(ctx, sid, c, k, offset, keep), entry };
}
static inline Item made(int sid, Geom g, const char *form, int k, std::vector<void *> *keep, int entry) { return Item{ made_picture(sid, g, form, k, keep), entry }; }

#endif
