/*
 * tests/native/fake_integral_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_integral_pictures,
 * hvq_window_pictures and hvq_rect_sums of the runtime (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and
 * tests/native/fake_integral.cpp) through include/hvqm4_amd.h.  It writes what it read back and judges nothing:
 * tests/test_integral_cpu.py compares with hvqm4_amd.integral.
 *
 *   fake_integral_driver <scenario> <outdir> <golden dir>
 *
 * The test writes into <outdir>: calls.txt and pictures.bin.  calls.txt, one fact per line:
 *   P <w> <h> <hs> <vs> <plane> <squares 0/1> <window 0/1> <mode> <rx> <ry> <k> <c> <invert>    a picture: its bytes are the next ones of
 *                                                                   pictures.bin; window 1: it goes through the window call under that rule
 *   R <i> <x0> <y0> <x1> <y1>                                        a rectangle of the tables of picture i
 * The driver builds no picture, rule or rectangle of its own, except the malformed ones of `refused`.
 *
 * Scenarios.  cases: the pictures of calls.txt in the caller's memory (src), ONE hvq_integral_pictures, then hvq_window_pictures over the
 * pictures that ask for it (equal rules share an entry; as few calls as their distinct rules allow, 64 a call), then ONE hvq_rect_sums
 * over the R lines, all on the same stream with no wait in between.  resident: the pictures of three clips where they lie, and the same
 * pictures inverted in the caller's memory, in one call; the rule is the first P line's, the plane k % 3 in the 4:4:4 clip and 0
 * elsewhere.  refused: every refusal of the header's lists.  nogpu: what a program linked without fake_integral.cpp gets.
 *
 * Outputs: sums.bin (the tables one behind the other, uint32), squares.bin (uint64, of the pictures that asked), window.bin (the
 * pictures of the window call), rects.bin (uint64 triples).  results.txt:
 *   G <label> <index> <guard>       1 when the 256 bytes before and behind that output still hold the sentinel
 *   P <clip> <form> <k>             resident: the picture behind output <index> (form pic or inv), in order
 *   R <label> <return code>         a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the outputs after refused calls
 */
#define DRIVER_NAME "fake_integral_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

struct Want { Geom g; int plane, squares, window; HvqWindowRule rule; std::vector<uint8_t> bytes; };
static std::vector<Want> g_pics;
static std::vector<int32_t> g_rects;

static void load_inputs()
{
    std::ifstream f(g_out + "/calls.txt");
    std::ifstream bin(g_out + "/pictures.bin", std::ios::binary);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "R") {
            for (int k = 0; k < 5; ++k) { int32_t v; in >> v; g_rects.push_back(v); }
        } else if (what == "P") {
            Want w;
            memset(&w.rule, 0, sizeof w.rule);
            in >> w.g.w >> w.g.h >> w.g.hs >> w.g.vs >> w.plane >> w.squares >> w.window >> w.rule.mode >> w.rule.rx >> w.rule.ry >> w.rule.k >> w.rule.c >> w.rule.invert;
            w.rule.plane = w.plane;
            w.bytes.resize(bytes_of(w.g));
            bin.read((char *)w.bytes.data(), (std::streamsize)w.bytes.size());
            if (!bin) { fprintf(stderr, DRIVER_NAME ": pictures.bin is short\n"); exit(2); }
            g_pics.push_back(w);
        }
        if (!in) { fprintf(stderr, DRIVER_NAME ": calls.txt: a short line: %s\n", line.c_str()); exit(2); }
    }
}

static size_t plane_samples(Geom g, int plane)
{
    return plane ? (size_t)(g.w >> (g.hs == 2)) * (size_t)(g.h >> (g.vs == 2)) : (size_t)g.w * g.h;
}

static FILE *out_file(const char *name)
{
    FILE *f = fopen((g_out + "/" + name).c_str(), "wb");
    if (!f) { fprintf(stderr, DRIVER_NAME ": cannot write %s\n", name); exit(2); }
    return f;
}

/* a room read back: its bytes into `f`, a G line about its guards */
static void write_room(FILE *f, const char *label, size_t index, uint8_t *room, size_t nb)
{
    std::vector<uint8_t> host(nb + 2 * GUARD);
    HIP(hipMemcpy(host.data(), room, host.size(), hipMemcpyDeviceToHost));
    int guard = 1;
    for (size_t g = 0; g < GUARD; ++g) guard &= host[g] == SENTINEL && host[GUARD + nb + g] == SENTINEL;
    if (fwrite(host.data() + GUARD, 1, nb, f) != nb) exit(2);
    fprintf(g_res, "G %s %zu %d\n", label, index, guard);
    HIP(hipFree(room));
}

struct One { int sid, k; const void *src; Geom g; int plane, squares, window; HvqWindowRule rule; };

/* ONE integral call, the window calls behind it, ONE rectangle call behind them, then the wait and the files */
static void integral_window_rects(HvqContext *ctx, const std::vector<One> &v, hipStream_t caller)
{
    const int n = (int)v.size();
    std::vector<int> sids, ords, planes;
    std::vector<const void *> src;
    std::vector<uint8_t *> sroom, qroom;
    std::vector<uint32_t *> sums;
    std::vector<uint64_t *> squares;
    std::vector<uint32_t> dims;
    for (const One &p : v) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src); planes.push_back(p.plane);
        const size_t N = plane_samples(p.g, p.plane);
        sroom.push_back(guarded_room(4u * N));
        sums.push_back((uint32_t *)(sroom.back() + GUARD));
        qroom.push_back(p.squares ? guarded_room(8u * N) : nullptr);
        squares.push_back(p.squares ? (uint64_t *)(qroom.back() + GUARD) : nullptr);
        dims.push_back((uint32_t)(p.plane ? p.g.w >> (p.g.hs == 2) : p.g.w));
        dims.push_back((uint32_t)(p.plane ? p.g.h >> (p.g.vs == 2) : p.g.h));
    }
    CHECK(hvq_integral_pictures(ctx, n, sids.data(), ords.data(), src.data(), planes.data(), sums.data(), squares.data(), caller));
    std::vector<int> wsid, word, wwhich;
    std::vector<const void *> wsrc;
    std::vector<const uint32_t *> wsums;
    std::vector<const uint64_t *> wsq;
    std::vector<HvqWindowRule> rules;
    std::vector<uint8_t *> wroom;
    std::vector<void *> dst;
    std::vector<size_t> wnb;
    size_t first = 0;                                                 /* of the window call that is being gathered */
    auto window_call = [&]() {
        if (first == wsid.size()) return;
        CHECK(hvq_window_pictures(ctx, (int)(wsid.size() - first), wsid.data() + first, word.data() + first, wsrc.data() + first, wsums.data() + first, wsq.data() + first,
                                  rules.data(), (int)rules.size(), wwhich.data() + first, dst.data() + first, caller));
        first = wsid.size();
        rules.clear();
    };
    for (int i = 0; i < n; ++i) {
        const One &p = v[(size_t)i];
        if (!p.window) continue;
        {
            size_t r = 0;
            while (r < rules.size() && memcmp(&rules[r], &p.rule, sizeof p.rule)) ++r;
            if (r == rules.size() && rules.size() == (size_t)HVQ_WIN_MAX_RULES) window_call();      /* a call takes 64 distinct rules */
        }
        wsid.push_back(p.sid); word.push_back(p.k); wsrc.push_back(p.src); wsums.push_back(sums[(size_t)i]); wsq.push_back(squares[(size_t)i]);
        size_t r = 0;
        while (r < rules.size() && memcmp(&rules[r], &p.rule, sizeof p.rule)) ++r;
        if (r == rules.size()) rules.push_back(p.rule);
        wwhich.push_back((int)r);
        wnb.push_back(bytes_of(p.g));
        wroom.push_back(guarded_room(wnb.back()));
        dst.push_back(wroom.back() + GUARD);
    }
    window_call();
    const int nrects = (int)(g_rects.size() / 5u);
    uint8_t *rroom = nullptr;
    void *drects = nullptr, *ddims = nullptr;
    if (nrects) {
        HIP(hipMalloc(&drects, g_rects.size() * 4u));
        HIP(hipMemcpy(drects, g_rects.data(), g_rects.size() * 4u, hipMemcpyHostToDevice));
        HIP(hipMalloc(&ddims, dims.size() * 4u));
        HIP(hipMemcpy(ddims, dims.data(), dims.size() * 4u, hipMemcpyHostToDevice));
        rroom = guarded_room(24u * (size_t)nrects);
        CHECK(hvq_rect_sums(ctx, n, nrects, (const int32_t *)drects, sums.data(), squares.data(), (const uint32_t *)ddims, (uint64_t *)(rroom + GUARD), caller));
    }
    HIP(hipStreamSynchronize(caller));
    FILE *fs = out_file("sums.bin"), *fq = out_file("squares.bin"), *fw = out_file("window.bin"), *fr = out_file("rects.bin");
    size_t nq = 0;
    for (int i = 0; i < n; ++i) {
        const size_t N = plane_samples(v[(size_t)i].g, v[(size_t)i].plane);
        if (qroom[(size_t)i]) write_room(fq, "squares", nq++, qroom[(size_t)i], 8u * N);
    }
    for (int i = 0; i < n; ++i) write_room(fs, "sums", (size_t)i, sroom[(size_t)i], 4u * plane_samples(v[(size_t)i].g, v[(size_t)i].plane));
    for (size_t i = 0; i < wroom.size(); ++i) write_room(fw, "window", i, wroom[i], wnb[i]);
    if (rroom) write_room(fr, "rects", 0, rroom, 24u * (size_t)nrects);
    fclose(fs); fclose(fq); fclose(fw); fclose(fr);
    if (drects) HIP(hipFree(drects));
    if (ddims) HIP(hipFree(ddims));
}

static void scenario_cases(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<One> v;
    std::map<std::string, int> streams;
    for (const Want &w : g_pics) {
        const std::string key = std::to_string(w.g.w) + "x" + std::to_string(w.g.h) + ":" + std::to_string(w.g.hs) + std::to_string(w.g.vs);
        if (!streams.count(key)) { streams[key] = hvq_stream_open(ctx, w.g.w, w.g.h, w.g.hs, w.g.vs, 1, 3); CHECK(streams[key]); }
        v.push_back(One{ streams[key], -1, uploaded(w.bytes, v.size() & 1 ? 16 : 0, &keep), w.g, w.plane, w.squares, w.window, w.rule });
    }
    integral_window_rects(ctx, v, caller);
    fprintf(g_res, "R cases/n0 %d\n", hvq_integral_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, caller));
    fprintf(g_res, "R cases/window_n0 %d\n", hvq_window_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, caller));
    uint32_t *one[1] = { (uint32_t *)16 };
    fprintf(g_res, "R cases/rects_0 %d\n", hvq_rect_sums(ctx, 1, 0, nullptr, one, nullptr, nullptr, nullptr, caller));
    for (void *p : keep) HIP(hipFree(p));
}

/* the rule comes from the first P line of calls.txt */
static void scenario_resident(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<One> v;
    for (const char *nm : { "crossplane420_64x48", "yuv422_296x160", "crossplane444_48x64" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int k = 0; k < (int)c.pics.size() && k < 3; ++k) {
            const Picture a = resident_picture(sid, c, k), b = inverted_picture(ctx, sid, c, k, k & 1 ? 16 : 0, &keep);
            HvqWindowRule r = g_pics[0].rule;
            r.plane = a.g.hs == 1 ? k % 3 : 0;
            v.push_back(One{ a.sid, a.k, a.src, a.g, r.plane, 1, 1, r });
            v.push_back(One{ b.sid, b.k, b.src, b.g, r.plane, 1, 1, r });
            fprintf(g_res, "P %s pic %d\nP %s inv %d\n", nm, k, nm, k);
        }
    }
    integral_window_rects(ctx, v, caller);
    for (void *p : keep) HIP(hipFree(p));
}

/* one picture, every call refused: the outputs keep their sentinel */
static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t sb = 4u * plane_samples(g, 0), qb = 8u * plane_samples(g, 0), pb = bytes_of(g), rb = 24u * 4u;
    uint8_t *room = guarded_room(2 * (sb + qb + pb) + rb, 0);
    uint32_t *S[2] = { (uint32_t *)room, (uint32_t *)(room + sb) };
    uint64_t *Q[2] = { (uint64_t *)(room + 2 * sb), (uint64_t *)(room + 2 * sb + qb) };
    void *D[2] = { room + 2 * (sb + qb), room + 2 * (sb + qb) + pb };
    uint64_t *O = (uint64_t *)(room + 2 * (sb + qb + pb));
    void *mem = nullptr;
    HIP(hipMalloc(&mem, pb + 32));
    const int32_t hrects[20] = { 0, 0, 0, 3, 3, 1, 0, 0, 3, 3, 0, 1, 1, 2, 2, 1, 1, 1, 2, 2 };
    const uint32_t hdims[4] = { 64, 48, 64, 48 };
    void *drects = nullptr, *ddims = nullptr;
    HIP(hipMalloc(&drects, sizeof hrects)); HIP(hipMemcpy(drects, hrects, sizeof hrects, hipMemcpyHostToDevice));
    HIP(hipMalloc(&ddims, sizeof hdims)); HIP(hipMemcpy(ddims, hdims, sizeof hdims, hipMemcpyHostToDevice));
    const int two[2] = { 0, 0 }, w_hi[2] = { 0, 1 }, w_lo[2] = { -1, 0 }, p_hi[2] = { 0, 3 }, p_lo[2] = { -1, 0 }, p_u[2] = { 0, 1 };
    uint32_t *Snull[2] = { S[0], nullptr }, *Smis[2] = { S[0], S[1] + 1 };
    uint64_t *Qmis[2] = { Q[0], Q[1] + 1 }, *Qnull[2] = { Q[0], nullptr };
    auto igl = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const int *planes, uint32_t *const *sums,
                   uint64_t *const *squares) {
        fprintf(g_res, "R refused/%s %d\n", label, hvq_integral_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), planes, sums, squares, caller));
    };
    igl("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, nullptr, S, Q);
    igl("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, nullptr, S, Q);
    igl("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, nullptr, S, Q);
    igl("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, nullptr, S, Q);
    igl("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, nullptr, S, Q);
    igl("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, nullptr, S, Q);
    igl("plane_3", ctx, 2, { sa, sa }, { 0, 1 }, {}, p_hi, S, Q);
    igl("plane_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, p_lo, S, Q);
    igl("null_sums", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, nullptr, Q);
    igl("null_table", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, Snull, Q);
    igl("misaligned_table", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, Smis, Q);
    igl("misaligned_squares", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, S, Qmis);
    igl("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, nullptr, S, Q);
    igl("negative_n", ctx, -1, { sa, sa }, { 0, 1 }, {}, nullptr, S, Q);
    const HvqWindowRule good = { 0, HVQ_WIN_THRESHOLD, 5, 5, 51, 7, 0, 0 }, plain = { 0, HVQ_WIN_MEAN, 5, 5, 0, 0, 0, 0 };
    auto win = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const uint32_t *const *sums,
                   const uint64_t *const *squares, const HvqWindowRule *rules, int nrules, const int *which, void *const *dst) {
        fprintf(g_res, "R refused/%s %d\n", label,
                hvq_window_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), sums, squares, rules, nrules, which, dst, caller));
    };
    void *Dnull[2] = { D[0], nullptr }, *Dmis[2] = { (uint8_t *)D[0] + 8, D[1] };
    win("w_null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, nullptr, D);
    win("w_bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, S, Q, &good, 1, nullptr, D);
    win("w_bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, S, Q, &good, 1, nullptr, D);
    win("w_misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, S, Q, &good, 1, nullptr, D);
    win("w_null_sums", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, Q, &good, 1, nullptr, D);
    win("w_null_table", ctx, 2, { sa, sa }, { 0, 1 }, {}, Snull, Q, &good, 1, nullptr, D);
    win("w_misaligned_table", ctx, 2, { sa, sa }, { 0, 1 }, {}, Smis, Q, &good, 1, nullptr, D);
    win("w_misaligned_squares", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Qmis, &good, 1, nullptr, D);
    win("w_squares_needed", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, nullptr, &good, 1, nullptr, D);
    win("w_squares_needed_one", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Qnull, &good, 1, nullptr, D);
    win("w_null_rules", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, nullptr, 1, nullptr, D);
    win("w_nrules_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 0, nullptr, D);
    {
        std::vector<HvqWindowRule> many(65, good);
        win("w_nrules_65", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, many.data(), 65, two, D);
    }
    win("w_which_high", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, w_hi, D);
    win("w_which_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, w_lo, D);
    win("w_null_dst", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, nullptr, nullptr);
    win("w_null_destination", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, nullptr, Dnull);
    win("w_misaligned_destination", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, nullptr, Dmis);
    win("w_too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, nullptr, D);
    win("w_negative_n", ctx, -1, { sa, sa }, { 0, 1 }, {}, S, Q, &good, 1, nullptr, D);
    {
        const HvqWindowRule chroma[2] = { good, { 1, HVQ_WIN_MEAN, 1, 1, 0, 0, 0, 0 } };      /* U of a 4:2:2 picture has not the size of Y */
        win("w_plane_not_of_y_size", ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, chroma, 2, p_u, D);
    }
    auto bad = [&](const char *label, HvqWindowRule r) {                        /* in the second entry of a table whose first is the only one used */
        const HvqWindowRule tab[2] = { good, r };
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_window_check(&tab[1]));
        win(label, ctx, 2, { sa, sa }, { 0, 1 }, {}, S, Q, tab, 2, two, D);
    };
    bad("r_plane_3", { 3, 0, 1, 1, 0, 0, 0, 0 }); bad("r_plane_negative", { -1, 0, 1, 1, 0, 0, 0, 0 }); bad("r_mode_3", { 0, 3, 1, 1, 0, 0, 0, 0 });
    bad("r_mode_negative", { 0, -1, 1, 1, 0, 0, 0, 0 }); bad("r_rx_8192", { 0, 0, 8192, 1, 0, 0, 0, 0 }); bad("r_ry_8192", { 0, 0, 1, 8192, 0, 0, 0, 0 });
    bad("r_rx_negative", { 0, 0, -1, 1, 0, 0, 0, 0 }); bad("r_ry_negative", { 0, 0, 1, -1, 0, 0, 0, 0 }); bad("r_k_1025", { 0, 2, 1, 1, 1025, 0, 0, 0 });
    bad("r_k_low", { 0, 2, 1, 1, -1025, 0, 0, 0 }); bad("r_c_256", { 0, 2, 1, 1, 0, 256, 0, 0 }); bad("r_c_low", { 0, 2, 1, 1, 0, -256, 0, 0 });
    bad("r_invert_2", { 0, 2, 1, 1, 0, 0, 2, 0 }); bad("r_invert_negative", { 0, 2, 1, 1, 0, 0, -1, 0 }); bad("r_pad", { 0, 0, 1, 1, 0, 0, 0, 1 });
    fprintf(g_res, "R refused/check_null %d\n", hvq_window_check(nullptr));
    fprintf(g_res, "R refused/check_good %d\n", hvq_window_check(&good));
    fprintf(g_res, "R refused/check_widest %d\n", hvq_window_check(std::vector<HvqWindowRule>{ { 2, 1, 8191, 8191, 1024, -255, 1, 0 } }.data()));
    auto rct = [&](const char *label, HvqContext *cx, int n, int nrects, const void *rects, const uint32_t *const *sums, const uint64_t *const *squares, const void *dims, void *out) {
        fprintf(g_res, "R refused/%s %d\n", label, hvq_rect_sums(cx, n, nrects, (const int32_t *)rects, sums, squares, (const uint32_t *)dims, (uint64_t *)out, caller));
    };
    rct("c_null_context", nullptr, 2, 4, drects, S, Q, ddims, O);
    rct("c_n_0", ctx, 0, 4, drects, S, Q, ddims, O);
    rct("c_too_many", ctx, 65536, 4, drects, S, Q, ddims, O);
    rct("c_negative_nrects", ctx, 2, -1, drects, S, Q, ddims, O);
    rct("c_too_many_rects", ctx, 2, (1 << 24) + 1, drects, S, Q, ddims, O);
    rct("c_null_rects", ctx, 2, 4, nullptr, S, Q, ddims, O);
    rct("c_misaligned_rects", ctx, 2, 3, (uint8_t *)drects + 2, S, Q, ddims, O);
    rct("c_null_dims", ctx, 2, 4, drects, S, Q, nullptr, O);
    rct("c_misaligned_dims", ctx, 1, 4, drects, S, Q, (uint8_t *)ddims + 2, O);
    rct("c_null_out", ctx, 2, 4, drects, S, Q, ddims, nullptr);
    rct("c_misaligned_out", ctx, 2, 3, drects, S, Q, ddims, (uint8_t *)O + 4);
    rct("c_null_sums", ctx, 2, 4, drects, nullptr, Q, ddims, O);
    rct("c_null_table", ctx, 2, 4, drects, Snull, Q, ddims, O);
    rct("c_misaligned_table", ctx, 2, 4, drects, Smis, Q, ddims, O);
    rct("c_misaligned_squares", ctx, 2, 4, drects, S, Qmis, ddims, O);
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(2 * (sb + qb + pb) + rb);
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed calls right after them work */
    const int sid2[2] = { sa, sa }, ord2[2] = { 0, 1 };
    fprintf(g_res, "R refused/then_ok %d\n", hvq_integral_pictures(ctx, 2, sid2, ord2, nullptr, nullptr, S, Q, caller));
    fprintf(g_res, "R refused/then_window_ok %d\n", hvq_window_pictures(ctx, 2, sid2, ord2, nullptr, S, Q, &good, 1, nullptr, D, caller));
    fprintf(g_res, "R refused/then_window_without_squares_ok %d\n", hvq_window_pictures(ctx, 2, sid2, ord2, nullptr, S, nullptr, &plain, 1, nullptr, D, caller));
    fprintf(g_res, "R refused/then_rects_ok %d\n", hvq_rect_sums(ctx, 2, 4, (const int32_t *)drects, S, Qnull, (const uint32_t *)ddims, O, caller));
    HIP(hipStreamSynchronize(caller));
    HIP(hipFree(room)); HIP(hipFree(mem)); HIP(hipFree(drects)); HIP(hipFree(ddims));
}

/* a program linked without fake_integral.cpp: the calls check their arguments first and then say that the kernels are missing */
static void scenario_nogpu(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t sb = 4u * plane_samples(g, 0), pb = bytes_of(g);
    uint8_t *room = guarded_room(sb + pb + 32, 0);
    uint32_t *S[1] = { (uint32_t *)room };
    void *D[1] = { room + sb };
    const HvqWindowRule good = { 0, HVQ_WIN_MEAN, 3, 3, 0, 0, 0, 0 }, bad = { 0, 5, 3, 3, 0, 0, 0, 0 };
    const int sid[1] = { sa }, ord[1] = { 0 }, p_hi[1] = { 3 };
    fprintf(g_res, "R nogpu/integral_bad_plane %d\n", hvq_integral_pictures(ctx, 1, sid, ord, nullptr, p_hi, S, nullptr, caller));
    fprintf(g_res, "R nogpu/integral %d\n", hvq_integral_pictures(ctx, 1, sid, ord, nullptr, nullptr, S, nullptr, caller));
    fprintf(g_res, "R nogpu/window_bad_rule %d\n", hvq_window_pictures(ctx, 1, sid, ord, nullptr, S, nullptr, &bad, 1, nullptr, D, caller));
    fprintf(g_res, "R nogpu/window %d\n", hvq_window_pictures(ctx, 1, sid, ord, nullptr, S, nullptr, &good, 1, nullptr, D, caller));
    fprintf(g_res, "R nogpu/rects_bad_out %d\n", hvq_rect_sums(ctx, 1, 1, (const int32_t *)D[0], S, nullptr, (const uint32_t *)D[0], nullptr, caller));
    fprintf(g_res, "R nogpu/rects %d\n", hvq_rect_sums(ctx, 1, 1, (const int32_t *)D[0], S, nullptr, (const uint32_t *)D[0], (uint64_t *)(room + sb + pb), caller));
    fprintf(g_res, "R nogpu/n0 %d\n", hvq_integral_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, caller));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(sb + pb + 32);
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S nogpu %zu %zu\n", same, back.size());
    HIP(hipFree(room));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_integral_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    load_inputs();
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_integral_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "cases") run_scenario(scenario_cases);
    else if (sc == "resident") run_scenario(scenario_resident);
    else if (sc == "refused") run_scenario(scenario_refused);
    else if (sc == "nogpu") run_scenario(scenario_nogpu);
    else { fprintf(stderr, "fake_integral_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
