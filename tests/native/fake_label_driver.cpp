/*
 * tests/native/fake_label_driver.cpp -- TEST INFRASTRUCTURE: a stand-alone program that drives hvq_label_pictures and
 * hvq_select_components of the runtime (hvqm4_amd/csrc/hvq_runtime.cpp, linked unchanged against the CPU fake device and
 * tests/native/fake_label.cpp) through include/hvqm4_amd.h.  It writes what it read back and judges nothing: tests/test_label_cpu.py
 * compares with hvqm4_amd.labels.
 *
 *   fake_label_driver <scenario> <outdir> <golden dir>
 *
 * The test writes into <outdir>: calls.txt and pictures.bin.  calls.txt, one fact per line:
 *   cap <cap>                                                       the room of every record table
 *   S <area_min> <area_max> <w_min> <w_max> <h_min> <h_max> <invert>   a selection; they are numbered from 0
 *   P <w> <h> <hs> <vs> <plane> <lo> <hi> <connectivity> <selection, or -1>   a picture: its bytes are the next ones of pictures.bin
 * The driver builds no picture, rule or selection of its own, except the malformed ones of `refused`.
 *
 * Scenarios.  cases: the pictures of calls.txt in the caller's memory (src), ONE hvq_label_pictures (equal rules share an entry), then
 * ONE hvq_select_components over the pictures that name a selection, on the same stream with no wait in between.  resident: the pictures
 * of three clips where they lie, and the same pictures inverted in the caller's memory, in one call; select behind it.  refused: every
 * refusal of the header's lists.  nogpu: what a program linked without fake_label.cpp gets.
 *
 * Outputs: labels.bin (the maps one behind the other, uint32), comps.bin (the record tables, uint64 [cap + 1][8] each, filled with the
 * sentinel byte before the call), select.bin (the pictures of the select call).  results.txt:
 *   G <label> <index> <guard>       1 when the 256 bytes before and behind that output still hold the sentinel
 *   P <clip> <form> <k>             resident: the picture behind output <index> (form pic or inv), in order
 *   R <label> <return code>         a return code the test wants to see
 *   S <label> <bytes that still hold the sentinel> <bytes>     the outputs after refused calls
 */
#define DRIVER_NAME "fake_label_driver"
#include "fake_slot_driver.h"

#include <fstream>
#include <sstream>

struct Want { Geom g; HvqLabelRule rule; int select; std::vector<uint8_t> bytes; };
static std::vector<Want> g_pics;
static std::vector<HvqSelect> g_sel;
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
        else if (what == "S") {
            HvqSelect s;
            memset(&s, 0, sizeof s);
            in >> s.area_min >> s.area_max >> s.w_min >> s.w_max >> s.h_min >> s.h_max >> s.invert;
            g_sel.push_back(s);
        } else if (what == "P") {
            Want w;
            in >> w.g.w >> w.g.h >> w.g.hs >> w.g.vs >> w.rule.plane >> w.rule.lo >> w.rule.hi >> w.rule.connectivity >> w.select;
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

struct One { int sid, k; const void *src; Geom g; HvqLabelRule rule; int select; };

/* ONE label call and ONE select call behind it, then the wait and the files */
static void label_and_select(HvqContext *ctx, const std::vector<One> &v, hipStream_t caller)
{
    const int n = (int)v.size();
    std::vector<int> sids, ords, which;
    std::vector<const void *> src;
    std::vector<HvqLabelRule> rules;
    std::vector<uint8_t *> lroom, croom;
    std::vector<uint32_t *> labels;
    std::vector<uint64_t *> comps;
    for (const One &p : v) {
        sids.push_back(p.sid); ords.push_back(p.k); src.push_back(p.src);
        size_t r = 0;
        while (r < rules.size() && memcmp(&rules[r], &p.rule, sizeof p.rule)) ++r;
        if (r == rules.size()) rules.push_back(p.rule);
        which.push_back((int)r);
        lroom.push_back(guarded_room(4u * plane_samples(p.g, p.rule.plane)));
        croom.push_back(guarded_room(64u * ((size_t)g_cap + 1u)));
        labels.push_back((uint32_t *)(lroom.back() + GUARD));
        comps.push_back((uint64_t *)(croom.back() + GUARD));
    }
    CHECK(hvq_label_pictures(ctx, n, sids.data(), ords.data(), src.data(), rules.data(), (int)rules.size(), which.data(), labels.data(), comps.data(), g_cap, caller));
    std::vector<int> ssid, swhich;
    std::vector<const uint32_t *> slab;
    std::vector<const uint64_t *> scomp;
    std::vector<uint8_t *> sroom;
    std::vector<void *> dst;
    std::vector<size_t> snb;
    for (int i = 0; i < n; ++i) {
        if (v[(size_t)i].select < 0) continue;
        ssid.push_back(sids[(size_t)i]); swhich.push_back(v[(size_t)i].select); slab.push_back(labels[(size_t)i]); scomp.push_back(comps[(size_t)i]);
        snb.push_back(bytes_of(v[(size_t)i].g));
        sroom.push_back(guarded_room(snb.back()));
        dst.push_back(sroom.back() + GUARD);
    }
    if (!ssid.empty())
        CHECK(hvq_select_components(ctx, (int)ssid.size(), ssid.data(), slab.data(), scomp.data(), g_cap, g_sel.data(), (int)g_sel.size(), swhich.data(), dst.data(), caller));
    HIP(hipStreamSynchronize(caller));
    FILE *fl = out_file("labels.bin"), *fc = out_file("comps.bin"), *fs = out_file("select.bin");
    for (int i = 0; i < n; ++i) {
        write_room(fl, "labels", (size_t)i, lroom[(size_t)i], 4u * plane_samples(v[(size_t)i].g, v[(size_t)i].rule.plane));
        write_room(fc, "comps", (size_t)i, croom[(size_t)i], 64u * ((size_t)g_cap + 1u));
    }
    for (size_t i = 0; i < sroom.size(); ++i) write_room(fs, "select", i, sroom[i], snb[i]);
    fclose(fl); fclose(fc); fclose(fs);
}

static void scenario_cases(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<One> v;
    std::map<std::string, int> streams;
    for (const Want &w : g_pics) {
        const std::string key = std::to_string(w.g.w) + "x" + std::to_string(w.g.h) + ":" + std::to_string(w.g.hs) + std::to_string(w.g.vs);
        if (!streams.count(key)) { streams[key] = hvq_stream_open(ctx, w.g.w, w.g.h, w.g.hs, w.g.vs, 1, 3); CHECK(streams[key]); }
        v.push_back(One{ streams[key], -1, uploaded(w.bytes, v.size() & 1 ? 16 : 0, &keep), w.g, w.rule, w.select });
    }
    label_and_select(ctx, v, caller);
    fprintf(g_res, "R cases/n0 %d\n", hvq_label_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, caller));
    fprintf(g_res, "R cases/select_n0 %d\n", hvq_select_components(ctx, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, caller));
    for (void *p : keep) HIP(hipFree(p));
}

/* the rule and the selection come from the first P line of calls.txt */
static void scenario_resident(HvqContext *&ctx, hipStream_t caller)
{
    std::vector<void *> keep;
    std::vector<One> v;
    for (const char *nm : { "crossplane420_64x48", "yuv422_296x160", "crossplane444_48x64" }) {
        const Clip &c = clip(nm);
        const int sid = decode(ctx, c);
        for (int k = 0; k < (int)c.pics.size() && k < 3; ++k) {
            const Picture a = resident_picture(sid, c, k), b = inverted_picture(ctx, sid, c, k, k & 1 ? 16 : 0, &keep);
            HvqLabelRule r = g_pics[0].rule;
            r.plane = k % 3;
            v.push_back(One{ a.sid, a.k, a.src, a.g, r, r.plane == 0 ? g_pics[0].select : -1 });
            v.push_back(One{ b.sid, b.k, b.src, b.g, r, r.plane == 0 ? g_pics[0].select : -1 });
            fprintf(g_res, "P %s pic %d\nP %s inv %d\n", nm, k, nm, k);
        }
    }
    label_and_select(ctx, v, caller);
    for (void *p : keep) HIP(hipFree(p));
}

/* one picture, every call refused: the three outputs keep their sentinel */
static void scenario_refused(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t lb = 4u * plane_samples(g, 0), cb = 64u * 9u, pb = bytes_of(g);
    uint8_t *room = guarded_room(2 * (lb + cb + pb), 0);
    uint32_t *L[2] = { (uint32_t *)room, (uint32_t *)(room + lb) };
    uint64_t *Cp[2] = { (uint64_t *)(room + 2 * lb), (uint64_t *)(room + 2 * lb + cb) };
    void *D[2] = { room + 2 * (lb + cb), room + 2 * (lb + cb) + pb };
    void *mem = nullptr;
    HIP(hipMalloc(&mem, pb + 32));
    const HvqLabelRule good = { 0, 255, 255, 8 };
    const HvqSelect sgood = { 0, 9, 0, 9, 0, 9, 0, 0 };
    const int two[2] = { 0, 0 }, w_hi[2] = { 0, 1 }, w_lo[2] = { -1, 0 };
    auto lab = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, std::vector<int> ords, std::vector<const void *> src, const HvqLabelRule *rules, int nrules,
                   const int *which, uint32_t *const *labels, uint64_t *const *comps, int cap) {
        fprintf(g_res, "R refused/%s %d\n", label, hvq_label_pictures(cx, n, sids.data(), ords.data(), src.empty() ? nullptr : src.data(), rules, nrules, which, labels, comps, cap, caller));
    };
    uint32_t *Lnull[2] = { L[0], nullptr }, *Lmis[2] = { L[0], L[1] + 1 };
    uint64_t *Cnull[2] = { nullptr, Cp[1] }, *Cmis[2] = { Cp[0] + 1, Cp[1] };
    lab("null_context", nullptr, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, Cp, 8);
    lab("bad_stream", ctx, 2, { sa, 99 }, { 0, 0 }, {}, &good, 1, nullptr, L, Cp, 8);
    lab("bad_ordinal", ctx, 2, { sa, sa }, { 0, 1000 }, {}, &good, 1, nullptr, L, Cp, 8);
    lab("misaligned_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, (uint8_t *)mem + 8 }, &good, 1, nullptr, L, Cp, 8);
    lab("src_with_ordinal", ctx, 2, { sa, sa }, { 0, 1 }, { nullptr, mem }, &good, 1, nullptr, L, Cp, 8);
    lab("minus_one_without_src", ctx, 2, { sa, sa }, { 0, -1 }, { nullptr, nullptr }, &good, 1, nullptr, L, Cp, 8);
    lab("null_rules", ctx, 2, { sa, sa }, { 0, 1 }, {}, nullptr, 1, nullptr, L, Cp, 8);
    lab("nrules_0", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 0, nullptr, L, Cp, 8);
    {
        std::vector<HvqLabelRule> many(65, good);
        lab("nrules_65", ctx, 2, { sa, sa }, { 0, 1 }, {}, many.data(), 65, two, L, Cp, 8);
    }
    lab("which_high", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_hi, L, Cp, 8);
    lab("which_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, w_lo, L, Cp, 8);
    lab("cap_negative", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, Cp, -1);
    lab("cap_beyond", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, Cp, HVQ_LBL_MAX_CAP + 1);
    lab("null_labels", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, nullptr, Cp, 8);
    lab("null_label_map", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, Lnull, Cp, 8);
    lab("misaligned_label_map", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, Lmis, Cp, 8);
    lab("null_comps", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, nullptr, 8);
    lab("null_record_table", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, Cnull, 8);
    lab("misaligned_record_table", ctx, 2, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, Cmis, 8);
    lab("too_many", ctx, 65536, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, Cp, 8);
    lab("negative_n", ctx, -1, { sa, sa }, { 0, 1 }, {}, &good, 1, nullptr, L, Cp, 8);
    auto bad = [&](const char *label, HvqLabelRule r) {                         /* in the second entry of a table whose first is the only one used */
        const HvqLabelRule tab[2] = { good, r };
        fprintf(g_res, "R refused/check_%s %d\n", label, hvq_label_check(&tab[1]));
        lab(label, ctx, 2, { sa, sa }, { 0, 1 }, {}, tab, 2, two, L, Cp, 8);
    };
    bad("plane_3", { 3, 0, 0, 8 }); bad("plane_negative", { -1, 0, 0, 8 }); bad("lo_above_hi", { 0, 9, 8, 8 }); bad("lo_negative", { 0, -1, 8, 8 });
    bad("hi_256", { 0, 0, 256, 8 }); bad("connectivity_6", { 0, 0, 0, 6 }); bad("connectivity_0", { 0, 0, 0, 0 });
    fprintf(g_res, "R refused/check_null %d\n", hvq_label_check(nullptr));
    fprintf(g_res, "R refused/check_good %d\n", hvq_label_check(&good));
    auto sel = [&](const char *label, HvqContext *cx, int n, std::vector<int> sids, const uint32_t *const *labels, const uint64_t *const *comps, int cap, const HvqSelect *s, int nsel,
                   const int *which, void *const *dst) {
        fprintf(g_res, "R refused/%s %d\n", label, hvq_select_components(cx, n, sids.data(), labels, comps, cap, s, nsel, which, dst, caller));
    };
    void *Dnull[2] = { D[0], nullptr }, *Dmis[2] = { (uint8_t *)D[0] + 8, D[1] };
    sel("s_null_context", nullptr, 2, { sa, sa }, L, Cp, 8, &sgood, 1, nullptr, D);
    sel("s_bad_stream", ctx, 2, { sa, 99 }, L, Cp, 8, &sgood, 1, nullptr, D);
    sel("s_null_labels", ctx, 2, { sa, sa }, nullptr, Cp, 8, &sgood, 1, nullptr, D);
    sel("s_null_label_map", ctx, 2, { sa, sa }, Lnull, Cp, 8, &sgood, 1, nullptr, D);
    sel("s_misaligned_label_map", ctx, 2, { sa, sa }, Lmis, Cp, 8, &sgood, 1, nullptr, D);
    sel("s_null_comps", ctx, 2, { sa, sa }, L, nullptr, 8, &sgood, 1, nullptr, D);
    sel("s_null_record_table", ctx, 2, { sa, sa }, L, Cnull, 8, &sgood, 1, nullptr, D);
    sel("s_misaligned_record_table", ctx, 2, { sa, sa }, L, Cmis, 8, &sgood, 1, nullptr, D);
    sel("s_cap_negative", ctx, 2, { sa, sa }, L, Cp, -1, &sgood, 1, nullptr, D);
    sel("s_cap_beyond", ctx, 2, { sa, sa }, L, Cp, HVQ_LBL_MAX_CAP + 1, &sgood, 1, nullptr, D);
    sel("s_null_sel", ctx, 2, { sa, sa }, L, Cp, 8, nullptr, 1, nullptr, D);
    sel("s_nsel_0", ctx, 2, { sa, sa }, L, Cp, 8, &sgood, 0, nullptr, D);
    {
        std::vector<HvqSelect> many(65, sgood);
        sel("s_nsel_65", ctx, 2, { sa, sa }, L, Cp, 8, many.data(), 65, two, D);
    }
    sel("s_which_high", ctx, 2, { sa, sa }, L, Cp, 8, &sgood, 1, w_hi, D);
    sel("s_which_negative", ctx, 2, { sa, sa }, L, Cp, 8, &sgood, 1, w_lo, D);
    sel("s_null_dst", ctx, 2, { sa, sa }, L, Cp, 8, &sgood, 1, nullptr, nullptr);
    sel("s_null_destination", ctx, 2, { sa, sa }, L, Cp, 8, &sgood, 1, nullptr, Dnull);
    sel("s_misaligned_destination", ctx, 2, { sa, sa }, L, Cp, 8, &sgood, 1, nullptr, Dmis);
    sel("s_too_many", ctx, 65536, { sa, sa }, L, Cp, 8, &sgood, 1, nullptr, D);
    sel("s_negative_n", ctx, -1, { sa, sa }, L, Cp, 8, &sgood, 1, nullptr, D);
    auto sbad = [&](const char *label, HvqSelect s) {
        const HvqSelect tab[2] = { sgood, s };
        sel(label, ctx, 2, { sa, sa }, L, Cp, 8, tab, 2, two, D);
    };
    sbad("s_area", { 5, 4, 0, 9, 0, 9, 0, 0 }); sbad("s_width", { 0, 9, 3, 2, 0, 9, 0, 0 }); sbad("s_height", { 0, 9, 0, 9, 9, 0, 0, 0 });
    sbad("s_invert_2", { 0, 9, 0, 9, 0, 9, 2, 0 }); sbad("s_pad", { 0, 9, 0, 9, 0, 9, 0, 1 });
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(2 * (lb + cb + pb));
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S refused %zu %zu\n", same, back.size());
    /* the well-formed calls right after them work */
    fprintf(g_res, "R refused/then_ok %d\n", hvq_label_pictures(ctx, 2, std::vector<int>{ sa, sa }.data(), std::vector<int>{ 0, 1 }.data(), nullptr, &good, 1, nullptr, L, Cp, 8, caller));
    fprintf(g_res, "R refused/then_select_ok %d\n", hvq_select_components(ctx, 2, std::vector<int>{ sa, sa }.data(), L, Cp, 8, &sgood, 1, nullptr, D, caller));
    HIP(hipStreamSynchronize(caller));
    HIP(hipFree(room));
    HIP(hipFree(mem));
}

/* a program linked without fake_label.cpp: both calls check their arguments first and then say that the kernels are missing */
static void scenario_nogpu(HvqContext *&ctx, hipStream_t caller)
{
    const Clip &a = clip("yuv422_64x48");
    const int sa = decode(ctx, a);
    const Geom g = geom_of(a);
    const size_t lb = 4u * plane_samples(g, 0), cb = 64u * 9u, pb = bytes_of(g);
    uint8_t *room = guarded_room(lb + cb + pb, 0);
    uint32_t *L[1] = { (uint32_t *)room };
    uint64_t *Cp[1] = { (uint64_t *)(room + lb) };
    void *D[1] = { room + lb + cb };
    const HvqLabelRule good = { 0, 255, 255, 8 }, bad = { 0, 255, 255, 5 };
    const HvqSelect sgood = { 0, 9, 0, 9, 0, 9, 0, 0 };
    const int sid[1] = { sa }, ord[1] = { 0 };
    fprintf(g_res, "R nogpu/label_bad_rule %d\n", hvq_label_pictures(ctx, 1, sid, ord, nullptr, &bad, 1, nullptr, L, Cp, 8, caller));
    fprintf(g_res, "R nogpu/label %d\n", hvq_label_pictures(ctx, 1, sid, ord, nullptr, &good, 1, nullptr, L, Cp, 8, caller));
    fprintf(g_res, "R nogpu/select_bad_cap %d\n", hvq_select_components(ctx, 1, sid, L, Cp, -1, &sgood, 1, nullptr, D, caller));
    fprintf(g_res, "R nogpu/select %d\n", hvq_select_components(ctx, 1, sid, L, Cp, 8, &sgood, 1, nullptr, D, caller));
    fprintf(g_res, "R nogpu/n0 %d\n", hvq_label_pictures(ctx, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, caller));
    HIP(hipStreamSynchronize(caller));
    std::vector<uint8_t> back(lb + cb + pb);
    HIP(hipMemcpy(back.data(), room, back.size(), hipMemcpyDeviceToHost));
    size_t same = 0;
    for (uint8_t x : back) same += x == SENTINEL;
    fprintf(g_res, "S nogpu %zu %zu\n", same, back.size());
    HIP(hipFree(room));
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: fake_label_driver <scenario> <outdir> <golden dir>\n"); return 2; }
    const std::string sc = argv[1];
    g_out = argv[2]; g_golden = argv[3];
    load_inputs();
    g_res = fopen((g_out + "/results.txt").c_str(), "w");
    if (!g_res) { fprintf(stderr, "fake_label_driver: cannot write into %s\n", g_out.c_str()); return 2; }
    if (sc == "cases") run_scenario(scenario_cases);
    else if (sc == "resident") run_scenario(scenario_resident);
    else if (sc == "refused") run_scenario(scenario_refused);
    else if (sc == "nogpu") run_scenario(scenario_nogpu);
    else { fprintf(stderr, "fake_label_driver: unknown scenario %s\n", sc.c_str()); return 2; }
    fake_drain_all();
    fclose(g_res);
    return 0;
}
