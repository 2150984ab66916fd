/*
 * tests/native/fake_corner_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_corner_pictures of the runtime
 * (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and tests/native/fake_corner.cpp) through
 * include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_corner_cpu.py compares with hvqm4_amd.corners.
 *
 *   fake_corner_driver <scenario> <outdir> <golden dir>
 *
 * The test writes into <outdir>: calls.txt and pictures.bin.  calls.txt, one fact per line:
 *   cap <cap>                                                       the room of every list
 *   P <w> <h> <hs> <vs> <plane> <mode> <radius> <k> <nms> <margin> <threshold> <response 0 / 1>   a picture: its bytes are the next ones
 *                                                                   of pictures.bin
 * The driver builds no picture or rule of its own, except the malformed ones of `refused`.
 *
 * Scenarios.  cases: the pictures of calls.txt in the caller's memory (src), ONE hvq_corner_pictures (equal rules share an entry).
 * resident: the pictures of three clips where they lie, and the same pictures inverted in the caller's memory, in one call, under the
 * rule of the first P line on the planes 0, 1, 2 in turn, every second one with a response map.  refused: every refusal of the header's
 * list.  nogpu: what a program linked without fake_corner.cpp gets.
 *
 * Outputs: mask.bin (the mask pictures one behind the other), points.bin (the lists, int64 [cap + 1][4] each, filled with the sentinel
 * byte before the call), rows.bin (uint32 [Ny + 1] each), response.bin (int64 [Ny][Nx] of the pictures that asked).  results.txt:
 *   G <label> <index> <guard>       1 when the 256 bytes before and behind that output still hold the sentinel
 *   P <clip> <form> <k>             resident: the picture behind output <index> (form pic or inv), in order
 *   R <label> <return code>         a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the outputs after refused calls
 */
#define DRIVER_NAME "fake_corner_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

struct Want { Geom g; HvqCornerRule rule; int response; std::vector<uint8_t> bytes; };
static std::vector<Want> g_pics;
static int g_cap = 0;

static void load_inputs()
{
    std::ifstream f(g_out + "/calls.txt");
    std::ifstream bin(g_out + "/pictures.bin", std::ios::binary);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "cap") in >> g_cap;
        else if (what == "P") {
            Want w;
            memset(&w.rule, 0, sizeof w.rule);
            long long threshold = 0;
            in >> w.g.w >> w.g.h >> w.g.hs >> w.g.vs >> w.rule.plane >> w.rule.mode >> w.rule.radius >> w.rule.k >> w.rule.nms >> w.rule.margin >> threshold >> w.response;
            w.rule.threshold = threshold;
            w.bytes.resize(bytes_of(w.g));
            bin.read((char *)w.bytes.data(), (std::streamsize)w.bytes.size());
            if (!bin) { fprintf(stderr, DRIVER_NAME ": pictures.bin is short\n"); exit(2); }
            g_pics.push_back(w);
        }
        if (!in) { fprintf(stderr, DRIVER_NAME ": calls.txt: a short line: %s\n", line.c_str()); exit(2); }
    }
}

static void plane_size(Geom g, int plane, size_t *nx, size_t *ny)
{
    *nx = plane ? (size_t)(g.w >> (g.hs == 2)) : (size_t)g.w;
    *ny = plane ? (size_t)(g.h >> (g.vs == 2)) : (size_t)g.h;
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

struct One { int sid, k; const void *src; Geom g; HvqCornerRule rule; int response; };

/* ONE call, then the wait and the files */
static void corners_of(HvqContext *ctx, const std::vector<One> &v, hipStream_t caller)
{
    const int n = (int)v.size();
    std::vector<int> sids, ords, which;
    std::vector<const void *> src;
    std::vector<HvqCornerRule> rules;
    std::vector<uint8_t *> mroom, proom, rroom, qroom;
    std::vector<uint8_t *> mask;
    std::vector<int64_t *> points, response;
    std::vector<uint32_t *> rows;
    bool any = false;
    for (const One &p : v) {
        size_t nx, ny;
        plane_size(p.g, p.rule.plane, &nx, &ny);
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src);
        size_t r = 0;
        while (r < rules.size() && memcmp(&rules[r], &p.rule, sizeof p.rule)) ++r;
        if (r == rules.size()) rules.push_back(p.rule);
        which.push_back((int)r);
        mroom.push_back(guarded_room(bytes_of(p.g)));
        proom.push_back(guarded_room(32u * ((size_t)g_cap + 1u)));
        rroom.push_back(guarded_room(4u * (ny + 1u)));
        qroom.push_back(p.response ? guarded_room(8u * nx * ny) : nullptr);
        mask.push_back(mroom.back() + GUARD);
        points.push_back((int64_t *)(proom.back() + GUARD));
        rows.push_back((uint32_t *)(rroom.back() + GUARD));
        response.push_back(p.response ? (int64_t *)(qroom.back() + GUARD) : nullptr);
        any |= p.response != 0;
    }
    CHECK(hvq_corner_pictures(ctx, n, sids.data(), ords.data(), src.data(), rules.data(), (int)rules.size(), which.data(), mask.data(), points.data(), rows.data(),
                              any ? response.data() : nullptr, g_cap, caller));
    HIP(hipStreamSynchronize(caller));
    FILE *fm = out_file("mask.bin"), *fp = out_file("points.bin"), *fr = out_file("rows.bin"), *fq = out_file("response.bin");
    for (int i = 0; i < n; ++i) {
        size_t nx, ny;
        plane_size(v[(size_t)i].g, v[(size_t)i].rule.plane, &nx, &ny);
        write_room(fm, "mask", (size_t)i, mroom[(size_t)i], bytes_of(v[(size_t)i].g));
        write_room(fp, "points", (size_t)i, proom[(size_t)i], 32u * ((size_t)g_cap + 1u));
        write_room(fr, "rows", (size_t)i, rroom[(size_t)i], 4u * (ny + 1u));
        if (qroom[(size_t)i]) write_room(fq, "response", (size_t)i, qroom[(size_t)i], 8u * nx * ny);
    }
    fclose(fm); fclose(fp); fclose(fr); fclose(fq);
}

static void scenario_cases(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<One> v;
    std::map<std::string, int> streams;
    for (const Want &w : g_pics) {
        const std::string key = std::to_string(w.g.w) + "x" + std::to_string(w.g.h) + ":" + std::to_string(w.g.hs) + std::to_string(w.g.vs);
        if (!streams.count(key)) { streams[key] = hvq_stream_open(ctx, w.g.w, w.g.h, w.g.hs, w.g.vs, 1, 3); CHECK(streams[key]); }
        v.push_back(One{ streams[key], -1, uploaded(w.bytes, v.size() & 1 ? 16 : 0, &keep), w.g, w.rule, w.response });
    }
    corners_of(ctx, v, caller);
    fprintf(g_res, "R cases/n0 %d\n", hvq_corner_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, caller));
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
            HvqCornerRule r = g_pics[0].rule;
            r.plane = k % 3;
            v.push_back(One{ a.sid, a.k, a.src, a.g, r, 1 });
            v.push_back(One{ b.sid, b.k, b.src, b.g, r, 0 });
            fprintf(g_res, "P %s pic %d\nP %s inv %d\n", nm, k, nm, k);
        }
    }
    corners_of(ctx, v, caller);
    for (void *p : keep) HIP(hipFree(p));
}

static HvqCornerRule rule_of(int plane, int mode, int radius, int k, int nms, int margin, int64_t threshold, int pad0 = 0, int pad1 = 0)
{
    HvqCornerRule r;
    r.plane = plane; r.mode = mode; r.radius = radius; r.k = k; r.nms = nms; r.margin = margin; r.pad[0] = pad0; r.pad[1] = pad1; r.threshold = threshold;
    return r;
}

/* one geometry, every call refused: the outputs keep their sentinel */
static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t pb = bytes_of(g), lb = 32u * 9u, rb = 4u * 64u, qb = 8u * 64u * 48u;      /* rows: 49 entries, rounded up to 16 bytes */
    const size_t each = pb + lb + rb + qb;
    uint8_t *room = guarded_room(2 * each, 0);
    uint8_t *M[2] = { room, room + each };
    int64_t *P[2] = { (int64_t *)(room + pb), (int64_t *)(room + each + pb) };
    uint32_t *Y[2] = { (uint32_t *)(room + pb + lb), (uint32_t *)(room + each + pb + lb) };
    int64_t *Q[2] = { (int64_t *)(room + pb + lb + rb), (int64_t *)(room + each + pb + lb + rb) };
    void *mem = nullptr;
    HIP(hipMalloc(&mem, pb + 32));
    const HvqCornerRule good = rule_of(0, HVQ_CRN_HARRIS, 1, 10, 3, 0, 1);
    const int two[2] = { 0, 0 }, w_hi[2] = { 0, 1 }, w_lo[2] = { -1, 0 };
    auto crn = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const HvqCornerRule *rules, int nrules,
                   const int *which, uint8_t *const *mask, int64_t *const *points, uint32_t *const *rows, int64_t *const *response, int cap) {
        fprintf(g_res, "R refused/%s %d\n", label,
                hvq_corner_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), rules, nrules, which, mask, points, rows, response, cap, caller));
    };
    uint8_t *Mnull[2] = { M[0], nullptr }, *Mmis[2] = { M[0], M[1] + 8 };
    int64_t *Pnull[2] = { nullptr, P[1] }, *Pmis[2] = { P[0] + 1, P[1] };
    uint32_t *Ynull[2] = { Y[0], nullptr }, *Ymis[2] = { Y[0] + 1, Y[1] };
    int64_t *Qmis[2] = { Q[0], Q[1] + 1 };
    crn("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Y, Q, 8);
    crn("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, &good, 1, nullptr, M, P, Y, Q, 8);
    crn("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, &good, 1, nullptr, M, P, Y, Q, 8);
    crn("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, &good, 1, nullptr, M, P, Y, Q, 8);
    crn("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, &good, 1, nullptr, M, P, Y, Q, 8);
    crn("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, &good, 1, nullptr, M, P, Y, Q, 8);
    crn("null_rules", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, 1, nullptr, M, P, Y, Q, 8);
    crn("nrules_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 0, nullptr, M, P, Y, Q, 8);
    {
        std::vector<HvqCornerRule> many(65, good);
        crn("nrules_65", ctx, 2, { sa, sa }, { 0, 1 }, {}, many.data(), 65, two, M, P, Y, Q, 8);
    }
    crn("which_high", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_hi, M, P, Y, Q, 8);
    crn("which_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_lo, M, P, Y, Q, 8);
    crn("cap_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Y, Q, -1);
    crn("cap_beyond", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Y, Q, HVQ_CRN_MAX_CAP + 1);
    crn("null_masks", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, nullptr, P, Y, Q, 8);
    crn("null_mask", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, Mnull, P, Y, Q, 8);
    crn("misaligned_mask", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, Mmis, P, Y, Q, 8);
    crn("null_points", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, nullptr, Y, Q, 8);
    crn("null_point_list", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, Pnull, Y, Q, 8);
    crn("misaligned_point_list", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, Pmis, Y, Q, 8);
    crn("null_rows", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, nullptr, Q, 8);
    crn("null_row_index", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Ynull, Q, 8);
    crn("misaligned_row_index", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Ymis, Q, 8);
    crn("misaligned_response", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Y, Qmis, 8);
    crn("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Y, Q, 8);
    crn("negative_n", ctx, -1, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, M, P, Y, Q, 8);
    auto bad = [&](const char *label, HvqCornerRule r) {                        /* in the second entry of a table whose first is the only one used */
        const HvqCornerRule tab[2] = { good, r };
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_corner_check(&tab[1]));
        crn(label, ctx, 2, { sa, sa }, { 0, 1 }, {}, tab, 2, two, M, P, Y, Q, 8);
    };
    bad("plane_3", rule_of(3, 0, 1, 10, 3, 0, 1)); bad("plane_negative", rule_of(-1, 0, 1, 10, 3, 0, 1)); bad("mode_2", rule_of(0, 2, 1, 0, 3, 0, 1));
    bad("mode_negative", rule_of(0, -1, 1, 0, 3, 0, 1)); bad("radius_0", rule_of(0, 0, 0, 10, 3, 0, 1)); bad("radius_4", rule_of(0, 0, 4, 10, 3, 0, 1));
    bad("k_65", rule_of(0, 0, 1, 65, 3, 0, 1)); bad("k_negative", rule_of(0, 0, 1, -1, 3, 0, 1)); bad("k_under_min_eigen", rule_of(0, 1, 1, 10, 3, 0, 1));
    bad("nms_8", rule_of(0, 0, 1, 10, 8, 0, 1)); bad("nms_negative", rule_of(0, 0, 1, 10, -1, 0, 1)); bad("margin_256", rule_of(0, 0, 1, 10, 3, 256, 1));
    bad("margin_negative", rule_of(0, 0, 1, 10, 3, -1, 1)); bad("threshold_0", rule_of(0, 0, 1, 10, 3, 0, 0)); bad("threshold_negative", rule_of(0, 0, 1, 10, 3, 0, -5));
    bad("pad_0", rule_of(0, 0, 1, 10, 3, 0, 1, 1, 0)); bad("pad_1", rule_of(0, 0, 1, 10, 3, 0, 1, 0, 1));
    fprintf(g_res, "R refused/check_null %d\n", hvq_corner_check(nullptr));
    fprintf(g_res, "R refused/check_good %d\n", hvq_corner_check(&good));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(2 * each);
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed call right after them works, with and without response maps */
    fprintf(g_res, "R refused/then_ok %d\n", hvq_corner_pictures(ctx, 2, std::vector<int>{ sa, sa }.data(), std::vector<int>{ 0, 1 }.data(), nullptr, &good, 1, nullptr, M, P, Y, Q, 8, caller));
    fprintf(g_res, "R refused/then_ok_without_response %d\n",
            hvq_corner_pictures(ctx, 2, std::vector<int>{ sa, sa }.data(), std::vector<int>{ 0, 1 }.data(), nullptr, &good, 1, nullptr, M, P, Y, nullptr, 8, caller));
    HIP(hipStreamSynchronize(caller));
    HIP(hipFree(room));
    HIP(hipFree(mem));
}

/* a program linked without fake_corner.cpp: the call checks its arguments first and then says that the kernels are missing */
static void scenario_nogpu(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t pb = bytes_of(g), lb = 32u * 9u, rb = 4u * 64u;
    uint8_t *room = guarded_room(pb + lb + rb, 0);
    uint8_t *M[1] = { room };
    int64_t *P[1] = { (int64_t *)(room + pb) };
    uint32_t *Y[1] = { (uint32_t *)(room + pb + lb) };
    const HvqCornerRule good = rule_of(0, HVQ_CRN_HARRIS, 1, 10, 3, 0, 1), bad = rule_of(0, HVQ_CRN_HARRIS, 4, 10, 3, 0, 1);
    const int sid[1] = { sa }, ord[1] = { 0 };
    fprintf(g_res, "R nogpu/bad_rule %d\n", hvq_corner_pictures(ctx, 1, sid, ord, nullptr, &bad, 1, nullptr, M, P, Y, nullptr, 8, caller));
    fprintf(g_res, "R nogpu/bad_cap %d\n", hvq_corner_pictures(ctx, 1, sid, ord, nullptr, &good, 1, nullptr, M, P, Y, nullptr, -1, caller));
    fprintf(g_res, "R nogpu/corners %d\n", hvq_corner_pictures(ctx, 1, sid, ord, nullptr, &good, 1, nullptr, M, P, Y, nullptr, 8, caller));
    fprintf(g_res, "R nogpu/n0 %d\n", hvq_corner_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, caller));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(pb + lb + rb);
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S nogpu %zu %zu\n", same, back.size());
    HIP(hipFree(room));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_corner_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    load_inputs();
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_corner_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "cases") run_scenario(scenario_cases);
    else if (sc == "resident") run_scenario(scenario_resident);
    else if (sc == "refused") run_scenario(scenario_refused);
    else if (sc == "nogpu") run_scenario(scenario_nogpu);
    else { fprintf(stderr, "fake_corner_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
