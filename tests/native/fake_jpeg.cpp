/*
 * tests/native/fake_jpeg.cpp -- TEST INFRASTRUCTURE: the CPU body of hvq_launch_jpeg (hvqm4_amd/csrc/hvq_jpeg.hip) for the CPU fake device.
 * Linked into the JPEG driver only (tests/test_jpeg_cpu.py); the other drivers link without it, and the runtime's weak reference then makes
 * hvq_encode_jpeg refuse.
 *
 * The three launches are queued on their stream as one operation; when its body runs it does what they do, in their order and with their
 * division of the work -- measure: every restart interval of every picture coded, only its stuffed length written to the scratch; lay out:
 * lengths to offsets, lengths[i], the header and EOI when the file fits; emit: every interval coded again and stored at its offset with
 * its RST marker -- in scalar loops: full 8 x 8 sums of the DCT, one 64-bit bit accumulator per interval.  It reaches every byte through
 * fake_span at that moment: the job table with the quantisers and headers behind it, the scratch, the three planes, lengths[i] and the
 * destination (its cap bytes, so that a store at or beyond cap is a bug found here, not memory damaged).  It checks that no byte at or
 * beyond cap is stored, that every byte of a fitting file is stored exactly once, and that nothing of a file that does not fit is.
 */
#include "fake_device.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hvqm4_amd/csrc/hvq_desc.h"
#include "../../hvqm4_amd/csrc/hvq_jpeg.h"

namespace {

struct Sink {                       /* a destination with its per-byte store counts */
    uint8_t *out; uint64_t cap; std::vector<uint8_t> stored; int job;
    void store(uint64_t at, uint8_t v)
    {
        if (at >= cap) fake_die("jpeg: job %d: a store at byte %llu, the capacity is %llu", job, (unsigned long long)at, (unsigned long long)cap);
        if (stored[at]++) fake_die("jpeg: job %d: byte %llu is stored twice", job, (unsigned long long)at);
        out[at] = v;
    }
};

struct Bits {                       /* the bits of one interval: whole bytes leave the accumulator stuffed */
    uint64_t acc = 0; unsigned n = 0; uint64_t count = 0; Sink *sink = nullptr; uint64_t at = 0;
    void byte(uint8_t b)
    {
        if (sink) sink->store(at + count, b);
        ++count;
        if (b == 0xFF) { if (sink) sink->store(at + count, 0); ++count; }
    }
    void put(uint32_t code, unsigned len)
    {
        acc = acc << len | code; n += len;
        while (n >= 8) { byte((uint8_t)(acc >> (n - 8))); n -= 8; }
    }
    void flush() { if (n) put((1u << (8 - n)) - 1u, 8 - n); }
};

int sample(const uint8_t *plane, int pw, int ph, int x, int y) { return plane[(size_t)(y < ph ? y : ph - 1) * pw + (x < pw ? x : pw - 1)]; }

void code_block(Bits &bits, const uint8_t *plane, int pw, int ph, int x0, int y0, const uint32_t *qpack, int tab, int *pred)
{
    int C[8][8], r[8][8], z[64];
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 4; ++n) { C[k][n] = HVQ_JPEG_C[k][n]; C[k][7 - n] = k & 1 ? -HVQ_JPEG_C[k][n] : HVQ_JPEG_C[k][n]; }
    for (int y = 0; y < 8; ++y)
        for (int k = 0; k < 8; ++k) {
            int a = 0;
            for (int n = 0; n < 8; ++n) a += C[k][n] * (sample(plane, pw, ph, x0 + n, y0 + y) - 128);
            r[y][k] = (a + 1024) >> 11;
        }
    int izz[64];
    for (int k = 0; k < 64; ++k) izz[HVQ_JPEG_ZZ[k]] = k;
    for (int k = 0; k < 8; ++k)
        for (int l = 0; l < 8; ++l) {
            int a = 0;
            for (int y = 0; y < 8; ++y) a += C[k][y] * r[y][l];
            z[izz[k * 8 + l]] = hvq_jpeg_quantise((a + 16384) >> 15, qpack[k * 8 + l]);
        }
    const int diff = z[0] - *pred;
    *pred = z[0];
    uint32_t s = hvq_jpeg_size(diff), c = HVQ_JPEG_CODES.dc[tab][s];
    if (s > 11 || !c) fake_die("jpeg: a DC difference of size %u", s);
    bits.put(c >> 8, c & 255u);
    if (s) bits.put((uint32_t)(diff < 0 ? diff + (1 << s) - 1 : diff), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        if (!z[k]) { ++run; continue; }
        for (; run >= 16; run -= 16) { c = HVQ_JPEG_CODES.ac[tab][0xF0]; bits.put(c >> 8, c & 255u); }
        s = hvq_jpeg_size(z[k]);
        c = HVQ_JPEG_CODES.ac[tab][run << 4 | s];
        if (s > 10 || !c) fake_die("jpeg: an AC coefficient of size %u", s);
        bits.put(c >> 8, c & 255u);
        bits.put((uint32_t)(z[k] < 0 ? z[k] + (1 << s) - 1 : z[k]), s);
        run = 0;
    }
    if (run) { c = HVQ_JPEG_CODES.ac[tab][0]; bits.put(c >> 8, c & 255u); }
}

/* one restart interval: its stuffed length; with a sink its bytes stored at `at` */
uint64_t code_interval(const HvqJpegJob &J, const uint8_t *src, const HvqJpegQuant *q, uint32_t j, Sink *sink, uint64_t at)
{
    const int w = (int)J.w, h = (int)J.h, hs = (int)J.hs, vs = (int)J.vs, cw = w / hs, ch = h / vs;
    const uint8_t *Y = src, *U = src + (size_t)w * h, *V = U + (size_t)cw * ch;
    Bits bits;
    bits.sink = sink; bits.at = at;
    int pred[3] = { 0, 0, 0 };
    for (int mx = 0; mx < (int)J.mw; ++mx) {
        for (int by = 0; by < vs; ++by)
            for (int bx = 0; bx < hs; ++bx) code_block(bits, Y, w, h, (mx * hs + bx) * 8, ((int)j * vs + by) * 8, q->q[0], 0, &pred[0]);
        code_block(bits, U, cw, ch, mx * 8, (int)j * 8, q->q[1], 1, &pred[1]);
        code_block(bits, V, cw, ch, mx * 8, (int)j * 8, q->q[1], 1, &pred[2]);
    }
    bits.flush();
    return bits.count;
}

}

extern "C" hipError_t hvq_launch_jpeg(const void *jobs_dev, int njobs, uint32_t max_mh, uint32_t quant_off, void *scratch, hipStream_t stream)
{
    if (njobs <= 0 || !max_mh) return hipSuccess;
    if (njobs > 65535) return hipErrorInvalidValue;
    return fake_enqueue(stream, "jpeg", [=]() {
        if (quant_off != (size_t)njobs * sizeof(HvqJpegJob)) fake_die("jpeg: the quantisers lie %u bytes into a table of %d jobs", quant_off, njobs);
        const uint8_t *tab = (const uint8_t *)fake_span(jobs_dev, quant_off + sizeof(HvqJpegQuant), "jpeg: the job records and the quantisers");
        const HvqJpegJob *jobs = (const HvqJpegJob *)tab;
        const HvqJpegQuant *q = (const HvqJpegQuant *)(tab + quant_off);
        std::vector<Sink> sinks((size_t)njobs);
        std::vector<uint32_t *> scr((size_t)njobs);
        std::vector<const uint8_t *> src((size_t)njobs);
        for (int k = 0; k < njobs; ++k) {
            const HvqJpegJob &J = jobs[k];
            if ((J.src | J.out) & 15u || J.len & 7u || !J.src || !J.out || !J.len) fake_die("jpeg: job %d: a null or misaligned address", k);
            if (!J.w || !J.h || J.w % 8u || J.h % 8u || J.w >= HVQ_JP_MAX_SIDE || J.h >= HVQ_JP_MAX_SIDE || J.hs < 1 || J.hs > 2 || J.vs < 1 || J.vs > 2)
                fake_die("jpeg: job %d: %u x %u sampled %u x %u", k, J.w, J.h, J.hs, J.vs);
            if (J.mw != hvq_jpeg_mw(J.w, J.hs) || J.mh != hvq_jpeg_mh(J.h, J.vs) || J.mh > max_mh) fake_die("jpeg: job %d: %u x %u MCUs, the grid has %u rows", k, J.mw, J.mh, max_mh);
            if (J.cap < HVQ_JPEG_HEADER_BYTES + 2u) fake_die("jpeg: job %d: a capacity of %llu", k, (unsigned long long)J.cap);
            scr[(size_t)k] = (uint32_t *)fake_span((uint32_t *)scratch + J.scr_first, ((size_t)J.mh + 1u) * 4u, "jpeg: the picture's scratch");
            const size_t pb = (size_t)J.w * J.h + 2u * (size_t)(J.w / J.hs) * (J.h / J.vs);
            src[(size_t)k] = (const uint8_t *)fake_span((const void *)(uintptr_t)J.src, pb, "jpeg: the picture");
            sinks[(size_t)k] = Sink{ (uint8_t *)fake_span((const void *)(uintptr_t)J.out, (size_t)J.cap, "jpeg: the destination"), J.cap, std::vector<uint8_t>((size_t)J.cap, 0), k };
        }
        /* 1. measure */
        for (int k = 0; k < njobs; ++k)
            for (uint32_t j = 0; j < max_mh; ++j) {
                if (j >= jobs[k].mh) break;                                      /* workgroups past the picture's last interval leave */
                scr[(size_t)k][1u + j] = (uint32_t)code_interval(jobs[k], src[(size_t)k], q, j, nullptr, 0);
            }
        /* 2. lay out */
        for (int k = 0; k < njobs; ++k) {
            const HvqJpegJob &J = jobs[k];
            uint64_t running = HVQ_JPEG_HEADER_BYTES;
            for (uint32_t j = 0; j < J.mh; ++j) {
                const uint32_t len = scr[(size_t)k][1u + j];
                scr[(size_t)k][1u + j] = (uint32_t)running;
                running += len + (j + 1u < J.mh ? 2u : 0u);
            }
            const uint64_t total = running + 2u;
            if (total >> 32) fake_die("jpeg: job %d: a file of %llu bytes", k, (unsigned long long)total);
            *(uint64_t *)fake_span((const void *)(uintptr_t)J.len, 8, "jpeg: lengths[i]") = total;
            scr[(size_t)k][0] = total <= J.cap;
            if (total > J.cap) continue;
            const uint8_t *hdr = (const uint8_t *)fake_span(tab + J.hdr_off, HVQ_JPEG_HEADER_BYTES, "jpeg: the picture's header");
            for (uint32_t i = 0; i < HVQ_JPEG_HEADER_BYTES; ++i) sinks[(size_t)k].store(i, hdr[i]);
            sinks[(size_t)k].store(total - 2u, 0xFF);
            sinks[(size_t)k].store(total - 1u, 0xD9);
        }
        /* 3. emit */
        for (int k = 0; k < njobs; ++k) {
            const HvqJpegJob &J = jobs[k];
            Sink &S = sinks[(size_t)k];
            const uint64_t total = *(const uint64_t *)(uintptr_t)J.len;
            if (!scr[(size_t)k][0]) {
                for (uint8_t n : S.stored) if (n) fake_die("jpeg: job %d: bytes of a file that does not fit were stored", k);
                continue;
            }
            for (uint32_t j = 0; j < J.mh; ++j) {
                const uint64_t at = scr[(size_t)k][1u + j], len = code_interval(J, src[(size_t)k], q, j, &S, at);
                if (j + 1u < J.mh) { S.store(at + len, 0xFF); S.store(at + len + 1u, (uint8_t)(0xD0u + (j & 7u))); }
            }
            for (uint64_t i = 0; i < J.cap; ++i)
                if (S.stored[i] != (i < total)) fake_die("jpeg: job %d: byte %llu of a file of %llu is stored %u times", k, (unsigned long long)i, (unsigned long long)total, S.stored[i]);
        }
    });
}
