#!/usr/bin/env python3
"""Generate tests/golden/bench_tools.json: what the trace summaries of the feature benchmarks (tools/*_bench.py) return for small synthetic
kernel traces, recorded from the tools as they stood at commit fcd8968bd3b4b889761d45e45924411cacad4b45, before tools/benchlib.py: every
tool had its own reader of the trace then.

    python tests/golden/make_bench_tools.py <a checkout of that commit>

`cases()` gives per summary function the launches of a trace in launch order, what the tool's child prints at --reps 3 (its plan) and the
results of earlier steps the summary looks at; `write_trace` writes the launches as a kernel trace the way rocprofv3 lays it out.  Both are
plain arithmetic, so tests/test_bench_tools.py makes the same traces again and checks today's tools against the recorded summaries.  A
block is one warm-up launch, an outlier, and three launches whose median, minimum and maximum differ; blocks alternate between the two
spellings of a kernel's name, with its signature and with a .kd suffix, and the _Float16 instantiations have the mangled name rocprofv3
leaves them with.  Recorded results only.
"""
import csv
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = "fcd8968bd3b4b889761d45e45924411cacad4b45"
REPS = 3
W, H = 640, 480
PIC = W * H * 3 // 2
COLUMNS = ("Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp", "VGPR_Count", "LDS_Block_Size", "Scratch_Size")
RESOURCES = {"hvq_metrics_kernel": (24, 1024, 0), "hvq_yuv_rgb_kernel": (32, 0, 0), "hvq_ssim_kernel": (56, 8192, 0), "hvq_histogram_kernel": (20, 12288, 0),
             "hvq_motion_kernel": (64, 16384, 0), "hvq_jpeg_code_kernel": (72, 3072, 0), "hvq_jpeg_layout_kernel": (16, 0, 0),
             "hvq_yuv_tensor_kernel": (40, 0, 0), "hvq_yuv_resample_kernel": (48, 20480, 0), "hvq_checksum_kernel": (28, 2048, 0),
             "hvq_checksum_finish_kernel": (12, 512, 0), "hvq_phash_cells_kernel": (36, 4096, 0), "hvq_phash_finish_kernel": (44, 8448, 0),
             "hvq_hash_nearest_kernel": (30, 0, 0), "hvq_scale_kernel": (38, 0, 0), "hvq_filter_kernel": (52, 30720, 0), "hvq_warp_kernel": (46, 40960, 16),
             "hvq_compose_kernel": (34, 0, 0), "hvq_recon_kernel": (96, 65536, 0)}
SIGNATURE = "(HvqJob const*, unsigned int)"


def block(kernel, calls=1 + REPS):
    """`calls` calls that launch the kernel, or each of the kernels, once"""
    return [k for _ in range(calls) for k in ([kernel] if isinstance(kernel, str) else kernel)]


def durations(b, per_call, launches):
    """of block b: the first call is the warm-up, slower than every other; the others spread above the block's own base.  A block of one
    call is a small launch of the set-up"""
    base = 100_000 + 7_919 * b
    spread = (4_321, 0, 1_234, 2_468, 617)
    if launches == per_call:
        return [2_000 + b] * launches
    return [base + 40_000 if j < per_call else base + 311 * (j % per_call) + spread[(j // per_call - 1) % len(spread)] for j in range(launches)]


def write_trace(trace_dir, blocks, name="7_kernel_trace.csv"):
    """blocks: lists of kernel names (with their template arguments) in launch order.  Launches of the decoder stand between the blocks,
    and the rows are written latest first: a reader has to pick and sort"""
    rows, t = [], 1_000_000_000
    for b, launches in enumerate(blocks):
        per_call = len(dict.fromkeys(launches))
        for kernel, ns in zip(["hvq_recon_kernel"] + launches, [777] + durations(b, per_call, len(launches))):
            base = kernel.split("<")[0]
            shown = kernel + ".kd" if b % 2 else ("void " if "<" in kernel else "") + kernel + SIGNATURE
            if "<_Float16>" in kernel:                                                # rocprofv3 leaves these instantiations mangled
                shown = f"_Z{len(base)}{base}IDF16_EvPK6HvqJobj"
            rows.append(("KERNEL_DISPATCH", shown, t, t + ns) + RESOURCES.get(base, (8, 0, 0)))
            t += ns + 1_500
    os.makedirs(os.path.join(trace_dir, "host"), exist_ok=True)
    with open(os.path.join(trace_dir, "host", name), "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(COLUMNS)
        w.writerows(reversed(rows))


def cases():
    """summary -> (tool, function, blocks of the trace, what the child prints, results of earlier steps, how the parent's function is called)"""
    n, per = 1024, 1 + REPS
    c = {}
    c["metrics"] = ("metrics_bench", "trace_summary", [block("hvq_metrics_kernel"), block("hvq_metrics_kernel"), block("hvq_yuv_rgb_kernel"), block("hvq_yuv_rgb_kernel")],
                    {"plan": [["metrics_all", "hvq_metrics_kernel", per, n, 2 * PIC], ["metrics_newest", "hvq_metrics_kernel", per, 128, 2 * PIC],
                              ["export_rgbp", "hvq_yuv_rgb_kernel", per, n, PIC + 3 * W * H], ["export_yuv444p", "hvq_yuv_rgb_kernel", per, n, PIC + 3 * W * H]]}, None, "plan")
    windows = 159 * 119 + 2 * 79 * 59                                                 # 8 x 8 windows 4 apart in 640x480 and in 320x240 twice
    c["ssim"] = ("ssim_bench", "trace_summary", [block("hvq_ssim_kernel"), block("hvq_ssim_kernel"), block("hvq_metrics_kernel")],
                 {"plan": [["ssim", "hvq_ssim_kernel", per, n, 2 * PIC], ["ssim_maps", "hvq_ssim_kernel", per, n, 2 * PIC + 4 * windows],
                           ["metrics", "hvq_metrics_kernel", per, n, 2 * PIC]]}, None, "plan")
    hist = [("values_natural", "hvq_histogram_kernel", 1), ("absdiff_natural", "hvq_histogram_kernel", 2), ("values_flat", "hvq_histogram_kernel", 1),
            ("absdiff_flat", "hvq_histogram_kernel", 2), ("metrics_zeros", "hvq_metrics_kernel", 1), ("metrics_pairs", "hvq_metrics_kernel", 2)]
    c["histogram"] = ("histogram_bench", "trace_summary", [block(k) for _l, k, _s in hist], {"plan": [[l, k, per, n, s * PIC] for l, k, s in hist]}, None, "plan")
    labels = [f"{content}_b{B}_r{R}" for B, R in ((16, 8), (16, 15), (8, 8)) for content in ("natural", "flat", "itself")]
    c["motion"] = ("motion_bench", "trace_summary", [block("hvq_motion_kernel") for _ in labels], {"plan": [[l, per, n] for l in labels]}, None, "plan")
    call = ["hvq_jpeg_code_kernel<false>", "hvq_jpeg_layout_kernel", "hvq_jpeg_code_kernel<true>"]
    c["jpeg"] = ("jpeg_bench", "trace_summary", [block(call), block(call)], {"plan": [["dense", per], ["natural", per]]}, None, "plan")
    identity = [block("hvq_yuv_tensor_kernel<float>", 1), block("hvq_yuv_rgb_kernel", 2 + REPS)] + \
        [block(f"hvq_yuv_tensor_kernel<{t}>", 2 + REPS) for t in ("float", "_Float16", "hvq_bf16")] + [block("hvq_yuv_rgb_kernel", 2 + REPS)]
    c["export_float"] = ("export_float_bench", "trace_summary", identity,
                         {"pictures": n, "size": f"{W}x{H}", "reps": REPS, "export_float_float32_call_ms": 1.5, "export_rgbp_call_ms": 0.75}, None, "pictures")
    legs = [f"{w}x{h}_{dt}_{leg}" for h, w in ((224, 224), (240, 320)) for dt in ("float32", "float16") for leg in ("a_tiled", "b_direct", "c_plain")]
    c["export_float_aa"] = ("export_float_bench", "aa_trace_summary",
                            [block(("hvq_yuv_tensor_kernel" if leg.endswith("c_plain") else "hvq_yuv_resample_kernel") + ("<float>" if "float32" in leg else "<_Float16>"))
                             for leg in legs], {"plan": [[leg, per] for leg in legs]}, None, "plan")
    c["checksum"] = ("checksum_bench", "trace_summary", [block(["hvq_checksum_kernel", "hvq_checksum_finish_kernel"]), block("hvq_metrics_kernel")],
                     {"launches": per, "pictures": n}, None, "printed")
    c["phash"] = ("phash_bench", "trace_summary",
                  [block(["hvq_phash_cells_kernel", "hvq_phash_finish_kernel"]), block("hvq_metrics_kernel"), block("hvq_hash_nearest_kernel")],
                  {"launches": per, "pictures": n, "nearest": 16384}, None, "printed")
    printed = {"launches": per, "pictures": n, "content": "natural"}
    c["scale"] = ("scale_bench", "trace_summary", [block("hvq_scale_kernel") for _ in range(6)] + [block("hvq_metrics_kernel")], printed, None, "printed")
    c["filter"] = ("filter_bench", "trace_summary", [block("hvq_filter_kernel") for _ in range(6)] + [block("hvq_scale_kernel"), block("hvq_metrics_kernel")],
                   printed, None, "printed")
    c["warp"] = ("warp_bench", "trace_summary", [block("hvq_warp_kernel") for _ in range(3 + 3 * 7)] + [block("hvq_scale_kernel")], printed, None, "printed")
    c["compose"] = ("compose_bench", "trace_summary", [block("hvq_scale_kernel", 1)] + [block("hvq_compose_kernel") for _ in range(8)] + [block("hvq_scale_kernel")],
                    printed, {"calls": {"cases": {"copy": {"torch_median_ms": 2.5}, "average8": {"torch_median_ms": 31.25}}}}, "compose")
    return c


def parent_arguments(how, printed, earlier):
    """the arguments after the trace directory that the functions of the parent commit take"""
    return {"plan": lambda: (printed["plan"],), "pictures": lambda: (printed["pictures"],), "printed": lambda: (printed,),
            "compose": lambda: (printed, earlier["calls"])}[how]()


def main():
    import tempfile
    parent = os.path.abspath(sys.argv[1])
    os.environ.pop("HVQM4_AMD_LIB", None)
    out = {"generator": "tests/golden/make_bench_tools.py", "recorded_from_commit": PARENT, "reps": REPS,
           "what": "per summary function of tools/*_bench.py: what it returned at that commit for the trace of make_bench_tools.cases()", "summaries": {}}
    for name, (tool, function, blocks, printed, earlier, how) in cases().items():
        spec = importlib.util.spec_from_file_location("parent_" + tool, os.path.join(parent, "tools", tool + ".py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        assert module.ROOT == parent and "tools.benchlib" not in sys.modules, "not a checkout of that commit"
        with tempfile.TemporaryDirectory() as d:
            write_trace(d, blocks)
            res = getattr(module, function)(d, *parent_arguments(how, printed, earlier))
        assert "error" not in res, (name, res)
        out["summaries"][name] = res
        print(name, len(json.dumps(res)))
    with open(os.path.join(HERE, "bench_tools.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote bench_tools.json")


if __name__ == "__main__":
    main()
