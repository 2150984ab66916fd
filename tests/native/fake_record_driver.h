/*
 * tests/native/fake_record_driver.h -- TEST INFRASTRUCTURE: what the drivers of the calls that read pictures and write records
 * (fake_{metrics,ssim,checksums,histograms,motion,jpeg,phash}_driver.cpp) have in common on top of fake_driver_common.h: the output of
 * a call's records and its read-back, the sentinel buffers of the `refused` scenario with their S line, and the R + E lines of a
 * refusal.  A driver defines DRIVER_NAME and includes this header; its own are the pictures of a call and what the test is told about
 * them, its call_* (the library call), the format of its record line and its scenarios, which it hands to driver_main.
 */
#ifndef FAKE_RECORD_DRIVER_H
#define FAKE_RECORD_DRIVER_H

#include "fake_driver_common.h"

/* the output of a call: `bytes` filled with 0xFF (the call must replace every one of them) */
static inline void *record_room(size_t bytes)
{
    void *out = nullptr;
    HIP(hipMalloc(&out, bytes));
    std::vector<uint8_t> ff(bytes, 0xFF);
    HIP(hipMemcpy(out, ff.data(), ff.size(), hipMemcpyHostToDevice));
    return out;
}

/* ... read back as `count` words once the caller's stream has been waited for, and freed */
template <class T>
static inline std::vector<T> take_records(T **out, size_t count)
{
    std::vector<T> host(count);
    HIP(hipMemcpy(host.data(), *out, count * sizeof(T), hipMemcpyDeviceToHost));
    HIP(hipFree(*out));
    *out = nullptr;
    return host;
}

/* The buffers the refused calls of a scenario are pointed at: filled with 0xA5, which every byte must still hold when the S line is
 * written; freed with the scenario */
struct Sentinels {
    std::vector<std::pair<void *, size_t>> rooms;
    void *room(size_t bytes)
    {
        void *d = nullptr;
        HIP(hipMalloc(&d, bytes));
        std::vector<uint8_t> sent(bytes, 0xA5);
        HIP(hipMemcpy(d, sent.data(), bytes, hipMemcpyHostToDevice));
        rooms.push_back({ d, bytes });
        return d;
    }
    void write(const char *label) const
    {
        size_t same = 0, total = 0;
        for (const auto &r : rooms) {
            std::vector<uint8_t> back(r.second);
            HIP(hipMemcpy(back.data(), r.first, back.size(), hipMemcpyDeviceToHost));
            for (uint8_t x : back) same += x == 0xA5;
            total += back.size();
        }
        fprintf(g_res, "S %s %zu %zu\n", label, same, total);
    }
    ~Sentinels() { for (const auto &r : rooms) HIP(hipFree(r.first)); }
};

/* a return code the test wants to see, and the library's words for it (to the end of the line) */
static inline void write_code(const char *group, const char *label, int rc)
{
    fprintf(g_res, "R %s/%s %d\nE %s/%s %s\n", group, label, rc, group, label, hvq_last_error_string());
}

#endif
