/*
 * hvqm4_amd.h -- batched, device-resident extension of the HVQM4 decode path.
 *
 * The SDK signatures (hvqm4.h) hand host pointers in and out, so every call pays PCIe for
 * whole pictures.  This API is what a player/transcoder binds for throughput: pictures stay
 * in HBM, any number of streams are decoded per launch, and the host entropy parse
 * (h4m_audio_decode.c:1970-2056, serial per stream) overlaps GPU work.  It replaces the
 * reference's `decode_video` loop (h4m:2078-2138): frame-buffer rotation becomes slot
 * assignment, and pictures with no mutual dependency (across streams, and B pictures /
 * the next anchor inside a stream) are reconstructed by ONE kernel launch.
 *
 * Plain C ABI: pointers and sizes only.  All functions return HVQ_OK (0) / a non-negative
 * result, or a negative HVQ_E_* code; hvq_last_error_string() describes the last failure.
 */
#ifndef HVQM4_AMD_H
#define HVQM4_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVQ_OK            0
#define HVQ_E_ARG        -1
#define HVQ_E_OVERFLOW   -2
#define HVQ_E_GEOMETRY   -3
#define HVQ_E_NOGPU      -4
#define HVQ_E_HIP        -5
#define HVQ_E_STATE      -6
#define HVQ_E_CONTAINER  -7   /* malformed .h4m file (every case the reference exits on) */
#define HVQ_E_UNSUPPORTED -8  /* a picture this back end refuses rather than decode differently from the reference: malformed input
                                 that had to be clamped (HVQM4_AMD_ALLOW_CLAMPED=1 decodes it), an overflow-symbol run that does not
                                 end inside its section, or a P picture with future-referencing macroblocks (h4m:2058-2061, decoded
                                 like the reference since round 3) whose previous buffer content has left the stream's slot ring.
                                 The picture is not decoded, `present` is untouched, the stream resumes at its next I picture; other
                                 streams of the batch are unaffected. */

#define HVQ_FRAME_I 0x10   /* container frame ids, h4m:2065-2070 */
#define HVQ_FRAME_P 0x20
#define HVQ_FRAME_B 0x30

typedef struct HvqContext HvqContext;

typedef struct HvqStats {
    uint64_t pictures;          /* pictures in the last flushed batch */
    uint64_t luma_pixels;       /* sum of w*h over them */
    uint64_t algorithmic_bytes; /* 1.5 B/px written + 1.5 B/px read for P/B */
    uint64_t descriptor_bytes;  /* blob bytes uploaded (not credited in the roofline) */
    uint32_t launches;          /* kernel launches per pass: launch groups x dependency levels x launch queues */
    uint32_t workgroups;        /* total workgroups per pass */
    double   parse_seconds;     /* host entropy-parse time accumulated by hvq_stream_submit */
    uint32_t flags_or;          /* OR of all blob header flags (HVQ_F_*) */
    uint32_t gpu_parsed;        /* pictures of the batch whose bitstream was parsed on the GPU */
    double   gpu_parse_ms;      /* device time of that parse launch (HIP events) */
    uint32_t gpu_parse_retried; /* of those, pictures the flat parse path handed to the chain decoder (unusual section layout,
                                   capacities, overflow groups at the caps) -- same result, slower */
    uint32_t dropped;           /* pictures of the batch that were not reconstructed: rejected, or behind a rejected picture of their stream */
    uint32_t launch_queues;     /* 1, or 2: a batch of 16 streams or more of one picture size deals its streams -- by work -- to two chains of
                                   launches on two HIP streams (a hardware queue each) that run side by side; HVQM4_AMD_QUEUES=1 / 2 forces either */
    uint64_t queue_bytes;       /* always 0 since round 6 (rounds 3-5: bytes of the two-pass variant's tile queues); kept for the layout */
    uint64_t copy_bytes;        /* hvq_submit_many_device / _async: bitstream bytes the library copied into its pinned arena, summed since
                                   the context was created (hvq_submit_many_arena copies nothing) */
    double   copy_seconds;      /* ... and the wall time its copy threads took over them: host_copy GB/s = copy_bytes / copy_seconds */
} HvqStats;

int  hvq_context_create(int device, HvqContext **out);
/* Launch queues a batch of this context may use: 2 (default: a batch of 16 streams or more of one picture size deals its dependency levels
 * to two HIP streams, HvqStats.launch_queues) or 1.  A process that runs TWO contexts on a GPU side by side (INTEGRATION.md "Two contexts per
 * GPU") sets 1 on both: the contexts are each other's second queue, four queues get in each other's way (157 against 171 Gpixel/s). */
int  hvq_context_set_launch_queues(HvqContext *ctx, int n);
/* Launch groups: a batch whose reuse window -- per stream the largest sum, over two consecutive dependency levels, of the bytes its pictures
 * write and read; summed over the streams -- exceeds `bytes` is split into G = ceil(window / bytes) groups of streams (never fewer than 8
 * streams per launch queue in a group); every launch queue runs all levels of group 0, then of group 1, ..., so what lies between an anchor's
 * write and its reads is one group's window, not the batch's.  0: never split.  Same pictures either way; HvqStats.launches counts G times
 * as many.  Takes effect at the next hvq_flush_begin.  hvq_context_launch_groups: G of the last flushed batch (0: none), or an error. */
int  hvq_context_set_group_bytes(HvqContext *ctx, uint64_t bytes);
int  hvq_context_launch_groups(HvqContext *ctx);
uint64_t hvq_launch_group_default_bytes(void);     /* what a new context carries */
/* the rule itself (pure): pictures [first[s], first[s + 1]) of `kinds` (0 I, 1 P, 2 B) and `levels` are stream s's; group_of (nstreams
 * entries) and window may be null -> G */
uint32_t hvq_launch_group_plan(uint32_t nstreams, const uint32_t *pic_bytes, const uint32_t *first, const uint8_t *kinds, const int32_t *levels,
                               uint64_t budget, uint32_t queues, uint16_t *group_of, uint64_t *window);
void hvq_context_destroy(HvqContext *ctx);

/* A stream = one clip.  `nslots` >= 3 picture buffers stay resident in HBM per stream (the
 * reference rotates exactly 3, h4m:2340-2350; more slots let later pictures start earlier). */
int  hvq_stream_open(HvqContext *ctx, int width, int height, int h_samp, int v_samp, int is_1_5, int nslots);
int  hvq_stream_close(HvqContext *ctx, int stream);
/* Host threads that share the entropy parse of ONE picture of this stream (its sections are independent bit buffers, h4m:1981-1993,
 * 2030-2044; same blob byte for byte): 1 (default) .. 8.  For callers with few streams -- hvq_stream_submit parses a stream's pictures one
 * after the other, hvq_submit_many parses STREAMS side by side.  The SDK entry points set 4 (HVQM4_AMD_SDK_PARSE_THREADS).  Returns the
 * count in effect. */
int  hvq_stream_set_parse_threads(HvqContext *ctx, int stream, int threads);
/* Host only: bytes of the picture ring hvq_stream_open would allocate ((nslots + 1) slots; 0: geometry refused).  The kernels
 * address reference pictures as ring base + 32-bit offset, so hvq_stream_open fails with HVQ_E_OVERFLOW from 4 GiB on. */
uint64_t hvq_stream_ring_bytes(int width, int height, int h_samp, int v_samp, int nslots);

/* Parse one picture (host) and queue it.  `pic` = picture data after the 4-byte disp_id,
 * `len` its length.  Returns the picture's ordinal in the stream (decode order). */
int  hvq_stream_submit(HvqContext *ctx, int stream, int frame_type, const uint8_t *pic, size_t len);

/* Same as hvq_stream_submit for `n` pictures, with the host entropy parse spread over `threads` worker
 * threads (pictures of one stream are parsed in order by one worker -- the parser carries the nest of the
 * last I picture; different streams run concurrently).  Pictures are queued in array order.  ordinals[i]
 * (may be NULL) receives picture i's ordinal.  Returns HVQ_OK or the first error. */
int  hvq_submit_many(HvqContext *ctx, int n, const int *streams, const int *frame_types,
                     const uint8_t *const *pics, const size_t *lens, int threads, int *ordinals);

/* GPU entropy parse: queue RAW picture bitstreams; hvq_flush uploads them and parses them on
 * the device (one workgroup per picture, hvq_gparse.hip), so no host core touches a bit of the stream.  Same
 * queueing semantics as hvq_submit_many.  A stream uses either the host parser or the GPU parser for its whole
 * lifetime (the host parser keeps the nest of the last I picture); lens[] must be the real picture lengths.
 * Errors of the device parse (HVQ_E_OVERFLOW, HVQ_E_ARG) are reported by hvq_flush.
 * The bitstreams are copied into the library's pinned arena before the call returns: `pics[i]` are the caller's again on return. */
int  hvq_submit_many_device(HvqContext *ctx, int n, const int *streams, const int *frame_types,
                            const uint8_t *const *pics, const size_t *lens, int *ordinals);
/* The same with the copy DEFERRED to a worker thread of the library: the call returns at once, so a streaming caller reaches
 * hvq_flush_end (and the batch in flight its reconstruction launches) without waiting for 160 MB of host memcpy.  `pics[i]` (and
 * the arrays) must stay readable and unchanged until the next hvq_flush_begin or hvq_sync, which joins the worker; an upload that
 * fails on the worker is reported there and drops the whole queued batch (its streams resume at their next I picture).
 * (Round 4 did this inside hvq_submit_many_device whenever a batch was in flight; since round 5 it is opt-in by name.
 * HVQM4_AMD_ASYNC_SUBMIT=1 restores the old behaviour of the plain call.) */
int  hvq_submit_many_device_async(HvqContext *ctx, int n, const int *streams, const int *frame_types,
                                  const uint8_t *const *pics, const size_t *lens, int *ordinals);
/* Zero-copy submit.  hvq_arena_reserve hands out `bytes` of the pinned (DMA-able) arena the library uploads from; the caller
 * writes its pictures there itself -- a container reader read()s file bytes straight into it -- at 256-byte aligned, ascending
 * offsets, picture i occupying hvq_arena_stride(lens[i]) bytes (its length plus the zero padding the device reader needs, which
 * the library writes).  hvq_submit_many_arena then queues them without touching a byte: no memcpy, no second pass over the
 * host's memory.  One reservation at a time; the pointer is valid until its submit (or the next hvq_flush_begin, which drops an
 * unsubmitted reservation).  Same queueing semantics and errors as hvq_submit_many_device. */
int  hvq_arena_reserve(HvqContext *ctx, size_t bytes, void **ptr);
size_t hvq_arena_stride(size_t len);
int  hvq_submit_many_arena(HvqContext *ctx, int n, const int *streams, const int *frame_types,
                           const size_t *offsets, const size_t *lens, int *ordinals);

/* Upload queued descriptors, group queued pictures into dependency levels, launch. Async. */
int  hvq_flush(HvqContext *ctx);

/* The same in two halves, for streaming.  hvq_flush_begin queues what needs no answer from the GPU (uploads, the
 * entropy-parse kernel) and returns; the queued batch is now "in flight" and the caller may already submit the NEXT
 * batch -- its bitstreams are copied and uploaded (second arena, copy stream) while this one is parsed.
 * hvq_flush_end takes the parse results, builds the launch tables and launches the reconstruction.  One batch can be
 * in flight; every call that needs its pictures (sync, read, replay, stats, close) ends it implicitly. */
int  hvq_flush_begin(HvqContext *ctx);
int  hvq_flush_end(HvqContext *ctx);
/* The streaming step in one call: end the batch in flight and begin the queued one -- hvq_flush_end + hvq_flush_begin in effect,
 * errors and state included (the first error of either half is returned) -- but with the queued batch's parse kernel launched
 * BEFORE the host takes the results of the batch in flight, so that the GPU parses batch k + 1 while the host builds the tables
 * of batch k, whose reconstruction launches line up behind that parse.  Taken when both batches are GPU-parsed throughout and the
 * queued batch's bitstreams are in the arena before the parse results of the batch in flight arrive; in every other case the two
 * halves run in the plain order.  A streaming loop is: submit(k + 1) [deferred or zero-copy], hvq_flush_next, use batch k.
 * HVQM4_AMD_FLUSH_NEXT=0: always the plain order. */
int  hvq_flush_next(HvqContext *ctx);
int  hvq_sync(HvqContext *ctx);

/* Re-run the launches of the last flush `reps` times (descriptors already resident in HBM), the launch queues running free.
 * *gpu_ms = elapsed time between HIP events recorded on the launch stream around all reps. */
int  hvq_replay(HvqContext *ctx, int reps, float *gpu_ms);
/* What a NEW batch costs behind its parse, repeated `reps` times: what = 1 -- every repetition forks and joins the launch queues
 * exactly as a flush does (the reconstruction stage of the product; bench.py's timed step); what = 0 -- hvq_replay: the launch queues
 * fork once and join once around all repetitions (a queue that is ahead runs into the next pass); what = 2 -- nothing, 0 ms (it timed
 * the queue build of the two-pass variant, deleted in round 6). */
int  hvq_replay_stage(HvqContext *ctx, int reps, int what, float *gpu_ms);

/* Copy a still-resident picture (Y|U|V, pic_bytes) to host memory; synchronises. */
int  hvq_read_picture(HvqContext *ctx, int stream, int ordinal, void *dst, size_t cap);
uint32_t hvq_stream_pic_bytes(HvqContext *ctx, int stream);

/* Bulk readback for the throughput path: `n` resident pictures to host memory, all copies queued on a stream of their own behind
 * the reconstruction, ONE synchronisation.  dst[i] receives hvq_stream_pic_bytes() bytes; pinned destinations
 * (hvq_pinned_alloc) make the copies asynchronous DMA. */
int  hvq_read_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, void *const *dst);
void *hvq_pinned_alloc(size_t bytes);
void hvq_pinned_free(void *p);
/* Device address of a resident picture for consumers on the GPU (valid until the stream's ring reuses the slot, `nslots`
 * pictures later at the earliest); order the consumer after hvq_sync().  hvq_export_pictures does the ordering itself. */
int  hvq_picture_device_ptr(HvqContext *ctx, int stream, int ordinal, const void **ptr);

/* Display epilogue of the reference player (dumpRGB, h4m:897-926) on the GPU: converts a resident 4:2:0
 * picture to interleaved RGB24 (w*h*3 bytes, float math identical to the reference) and copies it to host. */
int  hvq_read_picture_rgb(HvqContext *ctx, int stream, int ordinal, void *dst, size_t cap);
/* The same conversion for a picture in host memory (Y|U|V 4:2:0, width a multiple of 4, height even): upload, convert, download. */
int  hvq_convert_yuv420_rgb(HvqContext *ctx, const void *yuv, int width, int height, void *rgb);
/* Measurement helper: converts the newest resident picture of every open 4:2:0 stream in ONE launch, `reps`
 * times, timed with HIP events on the launch stream.  bytes_per_rep = 1.5 B/px read + 3 B/px written. */
int  hvq_rgb_bench(HvqContext *ctx, int reps, float *gpu_ms, uint64_t *bytes_per_rep, uint32_t *pictures);

/* Export of resident pictures into the caller's device memory: `n` pictures, of any streams, sizes and samplings, converted in ONE
 * kernel launch on the caller's HIP stream, without a host synchronisation.
 *   Formats: HVQ_FMT_RGB24 -- interleaved (HWC), h rows of w*3 bytes; HVQ_FMT_RGBP -- planar (CHW), three planes of h rows of w
 *   bytes; HVQ_FMT_YUV444P -- planar (CHW), Y copied, U and V replicated to full resolution.  RGB is the display epilogue's dumpRGB
 *   arithmetic (h4m:897-926, bit-exact); output sample (i, j) reads chroma sample [(i >> hshift) * (w >> wshift) + (j >> wshift)]
 *   -- dumpRGB itself at 4:2:0 (the reference converts only 4:2:0), the same rule with the stream's shifts at 4:2:2 and 4:4:4.
 *   dst[i]: rows `row_pitch` bytes apart, planes `plane_pitch` bytes apart (planar formats; ignored for RGB24); 0 = dense (w*3 or
 *   w; row_pitch * h).  ptr, row_pitch and plane_pitch must be multiples of 4, pitches at least the dense ones, planes must not
 *   overlap (plane_pitch >= row_pitch * h).  The destination must hold what these describe: the library cannot check its size.
 *   Pictures are looked up as hvq_read_pictures does: HVQ_E_STATE for a picture queued but not flushed, one whose slot was reused
 *   or that was dropped; HVQ_E_ARG for a bad stream, ordinal, format, null pointer, pitch or alignment.  Every argument is checked
 *   before anything is enqueued: a refused call enqueues nothing and leaves every destination untouched.  The batch in flight is
 *   ended only when a requested picture belongs to it, so `hvq_flush_next; export(batch k)` keeps overlapping.
 *   Ordering: `hip_stream` (NULL = the null stream) first waits for the reconstruction of every flushed picture and for the
 *   previous export (of whatever stream), then converts; the call returns at once.  Work the caller queues on `hip_stream` after
 *   the call sees the pictures; other streams order themselves after it with an event of their own.
 *   Slot safety: later work of the library that writes picture slots (flushes, hvq_replay, hvq_replay_stage) waits on the GPU for
 *   the exports before it; hvq_stream_close and hvq_context_destroy wait for them on the host before freeing a ring.  A picture
 *   is therefore safe to export until its slot is handed to a later picture, and the export reads it whole. */
#define HVQ_FMT_RGB24    0
#define HVQ_FMT_RGBP     1
#define HVQ_FMT_YUV444P  2
typedef struct HvqExportDst { void *ptr; int64_t row_pitch, plane_pitch; } HvqExportDst;     /* pitches in bytes; 0 = dense */
int  hvq_export_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, int format,
                         const HvqExportDst *dst, void *hip_stream);

/* Export of resident pictures as the float tensors a network eats: crop, bilinear resize, per-channel normalisation and the
 * conversion to float32 / float16 / bfloat16, planar RGB (CHW: three planes of out_h rows of out_w elements), in ONE kernel launch
 * for any mix of streams, crops and output sizes.  Lookup, HVQ_E_STATE cases, ordering and slot safety are hvq_export_pictures'
 * (the two kinds of export share one chain: each waits for the previous export of either kind).
 *   Arithmetic, all single precision with one rounding per operation (never fused):
 *   source   P_c(y, x), 0 <= y < crop_h, 0 <= x < crop_w: the uint8 HVQ_FMT_RGBP sample at luma position (crop_y + y, crop_x + x),
 *            as a float (crop offsets may be odd: the chroma index rule above takes care of them);
 *   columns  sx = (float)crop_w / (float)out_w;  fx = max((j + 0.5f) * sx - 0.5f, 0);  xa = min((int)floorf(fx), crop_w - 1);
 *            xb = min(xa + 1, crop_w - 1);  lx = fx - (float)xa;  rows likewise with sy, out_h, crop_h -> ya, yb, ly
 *            (half-sample centres, taps clamped to the crop: bilinear "crop, then resize" without antialiasing);
 *   blend    t = P(ya,xa) * (1 - lx) + P(ya,xb) * lx;  b = P(yb,xa) * (1 - lx) + P(yb,xb) * lx;  v = t * (1 - ly) + b * ly;
 *   output   o = v * mul[c] + add[c], c = R, G, B; the 16-bit types are rounded to nearest even from o.
 *   With out size == crop size the blend is the identity (v == P exactly) and the kernel streams.
 *   dst[i]: pitches in bytes, 0 = dense (out_w * element size; row_pitch * out_h); crop_w == 0 (with crop_x, crop_y, crop_h 0)
 *   takes the whole picture.  HVQ_E_ARG for a bad dtype, null pointer, non-finite mul / add, out_w or out_h outside [1, 16384], a
 *   crop that is empty or leaves the picture, pitches below dense, overlapping planes, or a pointer or pitch that is not a
 *   multiple of the element size.  16-byte stores are used when ptr and the pitches are multiples of 16 and out_w is a multiple of
 *   16 / element size; the values do not depend on it. */
#define HVQ_T_F32   0
#define HVQ_T_F16   1
#define HVQ_T_BF16  2
typedef struct HvqTensorDst {
    void *ptr; int64_t row_pitch, plane_pitch;      /* bytes; 0 = dense */
    int32_t out_w, out_h;
    int32_t crop_x, crop_y, crop_w, crop_h;         /* luma samples; crop_w == 0: the whole picture */
} HvqTensorDst;
int  hvq_export_tensors(HvqContext *ctx, int n, const int *streams, const int *ordinals, int dtype,
                        const float mul[3], const float add[3], const HvqTensorDst *dst, void *hip_stream);

/* The float export with a choice of resampling filter.  HVQ_FILTER_BILINEAR is hvq_export_tensors (the call forwards: same bits);
 * HVQ_FILTER_TRIANGLE is the antialiased resize of PIL / torch `antialias=True`: a separable triangle filter, horizontal first,
 * whose support grows with the downscale, so that every source sample of the crop contributes.  Use it when the output is
 * smaller than the crop (640x480 -> 224x224 skips more than half of the samples with two taps); for upscaling it is an
 * interpolation much like the bilinear one, at identity size it is the identity.  HvqTensorDst, lookup, HVQ_E_STATE cases,
 * argument checks ("a refused call enqueues nothing"), ordering and slot safety are hvq_export_tensors'; the call joins the same
 * export chain.  A bad `filter` is HVQ_E_ARG.
 *   Tables, per axis (n_src = crop size, n_out = output size, 0 <= j < n_out), computed on the host in DOUBLE, one rounding per
 *   operation, never contracted:
 *       scale   = n_src / n_out;   support = max(scale, 1.0);   c = scale * (j + 0.5)
 *       first_j = max((int)(c - support + 0.5), 0)                      (C truncation)
 *       end_j   = min((int)(c + support + 0.5), n_src);   count_j = end_j - first_j      (>= 1, <= 2 * ceil(support) + 1)
 *       u_k     = max(0.0, 1.0 - fabs((k + first_j - c + 0.5) / support)),   k = 0 .. count_j - 1
 *       t       = u_0 + u_1 + ...  (left to right);   w_j[k] = (float)(u_k / t)        (the only rounding to float32)
 *   Zero weights at the ends are kept (every term is >= 0: they cannot change a bit).
 *   Pixels, all float32, one rounding per operation, never fused; P_c(y, x) is hvq_export_tensors' source sample; wx / fx are the
 *   table of (crop_w, out_w), wy / fy that of (crop_h, out_h):
 *       h_c(y, j) = P_c(y, fx_j) * wx_j[0];   then for k = 1 .. :  h = h + P_c(y, fx_j + k) * wx_j[k]
 *       v_c(i, j) = h_c(fy_i, j) * wy_i[0];   then for k = 1 .. :  v = v + h_c(fy_i + k, j) * wy_i[k]
 *       o = v * mul[c] + add[c];   the 16-bit types are rounded to nearest even from o.
 *   At output size == crop size every row of weights is [1, 0], so v == P exactly: the bits of hvq_export_tensors.  Against torch's
 *   F.interpolate(mode="bilinear", antialias=True, align_corners=False), which builds its weights in float32, the values differ
 *   by a few thousandths of a 0..255 unit.
 *   HVQ_FILTER_TRIANGLE_DIRECT gives the same bits through the kernel's untiled body alone: for measurements and tests (the
 *   library picks the body per picture by itself). */
#define HVQ_FILTER_BILINEAR        0
#define HVQ_FILTER_TRIANGLE        1
#define HVQ_FILTER_TRIANGLE_DIRECT 0x101
int  hvq_export_resampled(HvqContext *ctx, int n, const int *streams, const int *ordinals, int dtype, int filter,
                          const float mul[3], const float add[3], const HvqTensorDst *dst, void *hip_stream);
/* Host only, no GPU needed: the table of one axis in CSR form -- first[n_out], count[n_out]; the weights of output j start at
 * sum(count[0 .. j)).  weights == NULL: only *weights_len = the number of weights is returned.  HVQ_E_ARG for n_src outside
 * [1, 65535] or n_out outside [1, 16384]; HVQ_E_OVERFLOW when weights_cap (in floats) is too small. */
int  hvq_resample_table(int n_src, int n_out, int32_t *first, int32_t *count, float *weights, size_t weights_cap, size_t *weights_len);
/* Host only: which body of the kernel HVQ_FILTER_TRIANGLE takes for a crop_w x crop_h -> out_w x out_h picture: the output rows per
 * tile (16 or 8) of the tiled body -- a downscale whose tiles' source rows fit its LDS budget -- or 0 for the direct body
 * (upscales, identity, very large ratios).  The values do not depend on it. */
int  hvq_resample_tile_rows(int crop_w, int crop_h, int out_w, int out_h);

/* Metrics of resident pictures, computed where they lie: for `n` pairs (a_i, b_i), of any streams, sizes and samplings, in ONE kernel
 * launch on the caller's HIP stream and without a host synchronisation, per plane p = Y, U, V over all samples of the plane
 *       sum_a = sum a     sum_b = sum b     sad = sum |a - b|     sse = sum (a - b)^2
 * as exact integers.  out: `n` records of uint64_t [3 planes Y, U, V][4] = { sum_a, sum_b, sad, sse }, 96 bytes each, dense, in call
 * order, in DEVICE memory; the call writes all 96 * n bytes whatever they held before (the caller does not zero them).  Mean and
 * variance of a plane, the mean absolute difference of two pictures (scene changes, near-duplicates) and PSNR follow from them.
 *   a_i = picture (streams[i], ordinals[i]).  Its reference b_i:
 *     ref[i].stream >= 0                 the resident picture (ref[i].stream, ref[i].ordinal), of any stream of the same width, height
 *                                        and sampling as a_i; ref[i].ptr must be NULL.  A picture against itself: sad = sse = 0;
 *     ref[i].stream == -1, ptr != NULL   the caller's device memory, laid out as hvq_picture_device_ptr lays a picture out (Y | U | V
 *                                        tightly packed, hvq_stream_pic_bytes long); ptr must be a multiple of 16.  The library
 *                                        cannot check its size; it is read when the work runs on `hip_stream`;
 *     ref[i].stream == -1, ptr == NULL   a picture of zeros: sum_b = 0, sad = sum_a, sse = sum a^2 (mean and variance);
 *     ref == NULL                        every picture against zeros.
 *   Lookup, HVQ_E_STATE cases (a or b queued but not flushed, slot reused, dropped), ordering and slot safety are
 *   hvq_export_pictures'; the batch in flight is ended only when an a_i or a resident b_i belongs to it; the call joins the same export
 *   chain (it waits for the previous export of any kind, later slot writers wait for it).  HVQ_E_ARG for a bad stream or ordinal, a
 *   geometry mismatch between a_i and b_i, ptr together with stream >= 0, a stream below -1, a ptr that is not a multiple of 16, a null
 *   `out` or one that is not a multiple of 8, n above 65535.  Every argument is checked before anything is enqueued: a refused call
 *   enqueues nothing and leaves `out` untouched.  HVQ_E_NOGPU (after those checks) from a build without the metrics kernel.
 *   The sums do not depend on the order the GPU adds them in: the same call gives the same bits every time. */
typedef struct HvqMetricsRef { int32_t stream, ordinal; const void *ptr; } HvqMetricsRef;
int  hvq_picture_metrics(HvqContext *ctx, int n, const int *streams, const int *ordinals,
                         const HvqMetricsRef *ref, uint64_t *out, void *hip_stream);

/* Windowed SSIM of resident pictures, computed where they lie: for `n` pairs (a_i, b_i), of any streams, sizes and samplings, in ONE kernel
 * launch on the caller's HIP stream and without a host synchronisation, per plane the exact fixed-point sum of the window values and
 * the number of windows, and on request the map of window values.  The per-window arithmetic is that of x264 / ffmpeg's `ssim` filter
 * for 8-bit pictures; this text is the authority.
 *   Per plane p = Y, U, V of W x H samples (the library's geometries make every W and H a multiple of 4):
 *   Blocks and windows.  bw = W / 4, bh = H / 4.  Block (r, c), 0 <= r < bh, 0 <= c < bw, is the 4 x 4 samples at rows 4r .. 4r + 3,
 *       columns 4c .. 4c + 3.  Window (i, j), 0 <= i < bh - 1, 0 <= j < bw - 1, is the 8 x 8 samples of blocks (i .. i + 1, j .. j + 1):
 *       windows step 4 samples in both directions.  rows = max(bh - 1, 0), cols = max(bw - 1, 0), windows = rows * cols.  A plane
 *       narrower or lower than 8 samples (the 4 x 4 chroma of an 8 x 8 4:2:0 picture) has no window: its record is { 0, 0 }, not an error.
 *   Window integers.  Over the 64 samples of the window, a from picture a and b from picture b:
 *       s1 = sum a     s2 = sum b     ss = sum (a^2 + b^2)     s12 = sum a b
 *       vars = 64 ss - s1^2 - s2^2          covar = 64 s12 - s1 s2
 *       A = 2 s1 s2 + 416     B = 2 covar + 235963     C = s1^2 + s2^2 + 416     D = vars + 235963
 *       416 = (int)(.01^2 255^2 64 + .5), 235963 = (int)(.03^2 255^2 64 63 + .5).  All of these fit a signed 32-bit integer: s1, s2 <=
 *       16320, ss <= 8 323 200, |A|, |B|, C, D < 2^30.  B is odd, so never 0; A, C and D are positive.
 *   Window value, in float32, one rounding per operation, nothing fused:  q = ((float)A * (float)B) / ((float)C * (float)D); the
 *       conversions round to nearest even, the division is the correctly rounded one.
 *   Exact reduction.  f = (int)rint(q * 16777216.0f): the product is exact (a power of two), rint rounds half to even, and for |q| >= 0.5
 *       the product is an integer already.  sum_f = sum of f over the plane's windows, a 64-bit integer: the record does not depend on
 *       the order the GPU adds in.  The mean SSIM of the plane is sum_f / (HVQ_SSIM_ONE * windows).  Identical planes: f == HVQ_SSIM_ONE
 *       in every window.
 *   out: `n` records of int64_t [3 planes Y, U, V][2] = { sum_f, windows }, 48 bytes each, dense, in call order, in DEVICE memory, a
 *       multiple of 8; the call writes all 48 * n bytes whatever they held before.  `windows` is counted by the kernel (every wave adds
 *       the number of windows it evaluated) and equals rows * cols.
 *   ref: HvqMetricsRef as for hvq_picture_metrics, its two non-trivial forms: stream >= 0 -- a resident picture of the same geometry, of
 *       any stream, ptr NULL; stream == -1 with ptr -- the caller's device memory, Y | U | V tightly packed, a multiple of 16.  SSIM
 *       against zeros means nothing: ref == NULL (with n > 0) and { -1, *, NULL } are HVQ_E_ARG.
 *   maps: NULL, or `n` pointers, each NULL or a device pointer that is a multiple of 4 to hvq_ssim_windows(...) floats: the windows of Y,
 *       then U, then V, each plane row-major rows x cols, dense.  Element (i, j) is the q of window (i, j), the bits of the float before
 *       scaling.  Every element is written exactly once, nothing outside those floats is written.
 *   Lookup, HVQ_E_STATE cases, n <= 65535, the checks of `ref`, "every argument is checked before anything is enqueued: a refused call
 *   leaves `out` and every map untouched", ending the batch in flight only when a requested picture belongs to it, ordering on
 *   `hip_stream`, membership of the export chain and slot safety are hvq_picture_metrics'.  A NULL context is HVQ_E_ARG.  HVQ_E_NOGPU
 *   (after those checks) from a build without the SSIM kernel. */
#define HVQ_SSIM_ONE 16777216
/* host only: rows / cols of windows per plane, dims[p] = { rows, cols } (dims may be NULL); returns the total (>= 0), or HVQ_E_GEOMETRY
 * for a geometry hvq_stream_open refuses */
int  hvq_ssim_windows(int width, int height, int h_samp, int v_samp, int32_t dims[3][2]);
int  hvq_picture_ssim(HvqContext *ctx, int n, const int *streams, const int *ordinals, const HvqMetricsRef *ref,
                      int64_t *out, float *const *maps, void *hip_stream);

/* Checksums of resident pictures, computed where they lie: for `n` pictures, of any streams, sizes and samplings, in one kernel launch and
 * a tiny finishing launch behind it, on the caller's HIP stream and without a host synchronisation, zlib's CRC-32 and Adler-32 of every
 * plane and of the whole picture.  "Is this picture bit for bit the expected one?" is answered by comparing 4-byte values; no picture
 * crosses PCIe.  This text is the authority for the values; it makes no claim about the output of any muxer or tool.
 *   A plane is its samples, rows tightly packed, exactly as they lie in the slot (the library's geometries make every plane a multiple of
 *   16 bytes); `picture` is the bytes Y | U | V, what hvq_read_picture returns: crc32_picture == zlib's crc32 of that buffer.
 *   CRC-32 of the bytes m_0 .. m_(L-1): r = 0xFFFFFFFF; per byte r ^= m_i, then eight times r = (r >> 1) ^ (0xEDB88320 & -(r & 1)); the value
 *       is r ^ 0xFFFFFFFF (the reflected polynomial 0xEDB88320, initial register and final xor 0xFFFFFFFF: zlib's crc32(0, m, L)).
 *   Adler-32: lo = (1 + sum m_i) mod 65521, hi = (L + sum (L - i) m_i) mod 65521, i from 0; the value is hi << 16 | lo (seed 1, modulus
 *       65521: zlib's adler32(1, m, L)).
 *   Both are computed exactly in parallel -- the CRC register is linear over GF(2), Adler's halves are integer sums reduced once at the
 *   end -- so the values do not depend on the order the GPU combines partial results in: the same call gives the same bits every time.
 *   out: `n` records of uint64_t [8] = { crc32_Y, crc32_U, crc32_V, crc32_picture, adler32_Y, adler32_U, adler32_V, adler32_picture }, 64
 *       bytes each, dense, in call order, in DEVICE memory, a multiple of 8; every value lies in [0, 2^32); the call writes all 64 * n
 *       bytes whatever they held before.
 *   a_i = the resident picture (streams[i], ordinals[i]).  If src != NULL and src[i] != NULL, a_i is the caller's device memory instead,
 *       laid out as a picture of streams[i] (Y | U | V tightly packed, hvq_stream_pic_bytes long): src[i] must be a multiple of 16 and
 *       ordinals[i] must be -1; the library cannot check its size; it is read when the work runs on `hip_stream`.
 *   Lookup, HVQ_E_STATE cases, n <= 65535, "every argument is checked before anything is enqueued: a refused call leaves `out`
 *   untouched", ending the batch in flight only when a requested picture belongs to it, ordering on `hip_stream`, membership of the export
 *   chain and slot safety are hvq_picture_metrics'.  HVQ_E_ARG for a NULL context, a bad stream or ordinal, a src[i] that is not a multiple
 *   of 16 or comes with an ordinal other than -1, a null `out` or one that is not a multiple of 8.  n == 0 is HVQ_OK and does nothing.
 *   HVQ_E_NOGPU (after those checks) from a build without the checksum kernel. */
#define HVQ_CK_CRC32_Y 0
#define HVQ_CK_CRC32_U 1
#define HVQ_CK_CRC32_V 2
#define HVQ_CK_CRC32_PICTURE 3
#define HVQ_CK_ADLER32_Y 4
#define HVQ_CK_ADLER32_U 5
#define HVQ_CK_ADLER32_V 6
#define HVQ_CK_ADLER32_PICTURE 7
int  hvq_picture_checksums(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src, uint64_t *out,
                           void *hip_stream);
/* Host only, no GPU needed, zlib's crc32_combine / adler32_combine: the checksum of A | B from the checksums of A and of B and the length
 * of B in bytes -- a clip's running checksum from its pictures', a picture's from its planes'. */
uint32_t hvq_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
uint32_t hvq_adler32_combine(uint32_t a, uint32_t b, uint64_t len_b);

/* Histograms of resident pictures, computed where they lie: for `n` pictures, of any streams, sizes and samplings, in ONE kernel launch on
 * the caller's HIP stream and without a host synchronisation, per plane p = Y, U, V the 256-bin histogram of its samples as exact
 * integers.  The distribution is what the sums of hvq_picture_metrics average away: median and percentiles, exposure and black-frame
 * checks, Otsu thresholds, equalisation tables, scene cuts by histogram distance; and, of a picture against its reference, the maximum
 * absolute error and the error percentiles.
 *   mode HVQ_HIST_VALUES    out[p][v] = the number of samples of plane p of a_i that equal v.  ref must be NULL.
 *   mode HVQ_HIST_ABSDIFF   out[p][d] = the number of positions of plane p where |a_i - b_i| equals d.  ref gives b_i.
 *   Identities, in every mode:    sum over v of out[p][v] = the samples of plane p;
 *       in HVQ_HIST_VALUES:       sum v out[p][v] = sum_a of hvq_picture_metrics;
 *       in HVQ_HIST_ABSDIFF:      sum d out[p][d] = sad and sum d^2 out[p][d] = sse of hvq_picture_metrics for the same pair; a picture
 *                                 against itself has every position in bin 0.
 *   The counts are integers added with integer atomics: the record does not depend on the order the GPU adds in, the same call gives the
 *   same bits every time.
 *   out: `n` records of uint32_t [3 planes Y, U, V][HVQ_HIST_BINS], 3072 bytes each, dense, in call order, in DEVICE memory, a non-null
 *       multiple of 4; the call writes all 3072 * n bytes whatever they held before (the caller does not zero them).  32 bits hold every
 *       count: the largest plane the library opens is 8192 x 8192 = 2^26 samples.
 *   a_i = the resident picture (streams[i], ordinals[i]).  If src != NULL and src[i] != NULL, a_i is the caller's device memory instead,
 *       laid out as a picture of streams[i] (Y | U | V tightly packed, hvq_stream_pic_bytes long): src[i] must be a multiple of 16 and
 *       ordinals[i] must be -1; the library cannot check its size; it is read when the work runs on `hip_stream`
 *       (hvq_picture_checksums' src).
 *   ref: HvqMetricsRef as for hvq_picture_ssim, its two non-trivial forms: stream >= 0 -- a resident picture of the same width, height and
 *       sampling as streams[i], of any stream, ptr NULL; stream == -1 with ptr -- the caller's device memory, Y | U | V tightly packed, a
 *       multiple of 16.  |a - 0| is a: in HVQ_HIST_ABSDIFF ref == NULL (with n > 0) and an entry { -1, *, NULL } are HVQ_E_ARG.
 *   Lookup, HVQ_E_STATE cases (a or b queued but not flushed, slot reused, dropped), ordering on `hip_stream`, membership of the export
 *   chain and slot safety are hvq_picture_metrics'; the batch in flight is ended only when a resident a_i or a resident b_i belongs to
 *   it.  HVQ_E_ARG for a NULL context, a bad mode, a ref in HVQ_HIST_VALUES, a bad stream or ordinal, a src[i] that is not a multiple of 16
 *   or comes with an ordinal other than -1, the refusals of `ref` above and of hvq_picture_metrics (geometry mismatch, ptr together with
 *   stream >= 0, a stream below -1, a ptr that is not a multiple of 16), a null `out` or one that is not a multiple of 4, n above 65535.
 *   n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is enqueued: a refused call enqueues nothing and
 *   leaves `out` untouched.  HVQ_E_NOGPU (after those checks) from a build without the histogram kernel. */
#define HVQ_HIST_BINS     256
#define HVQ_HIST_VALUES   0      /* bin v counts the samples of a equal to v            */
#define HVQ_HIST_ABSDIFF  1      /* bin d counts the positions where |a - b| equals d   */
int  hvq_picture_histograms(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src, int mode,
                            const HvqMetricsRef *ref, uint32_t *out, void *hip_stream);

/* Block-matching motion fields between resident pictures, computed where they lie: for `n` pictures, of any streams and sizes, in ONE
 * kernel launch on the caller's HIP stream and without a host synchronisation, per block of picture a_i the displacement at which the
 * reference b_i looks most like it.  Full search on the LUMA plane only; a is W x H luma samples, b has the same geometry.
 *   Blocks.      block B is 8 or 16; rows = H / B, cols = W / B; block (r, c) is the B x B samples of a whose top-left corner is
 *                (y0, x0) = (B r, B c).  Widths and heights are multiples of 8: B = 8 always tiles.  B = 16 on a stream whose width or
 *                height is not a multiple of 16 is HVQ_E_ARG for the whole call: no sample is silently left out.
 *   Candidates.  radius R, 0 <= R <= HVQ_MOTION_MAX_RADIUS.  The candidates of a block are the displacements (dy, dx) with |dy| <= R and
 *                |dx| <= R whose displaced block lies wholly inside the picture: 0 <= y0 + dy, y0 + dy + B <= H, 0 <= x0 + dx,
 *                x0 + dx + B <= W.  No padding; nothing outside plane Y of b is read.  (0, 0) is always a candidate.
 *   Cost.        cost(dy, dx) = sum over 0 <= i, j < B of |a[y0 + i][x0 + j] - b[y0 + dy + i][x0 + dx + j]|, at most 65280.
 *   Winner.      the candidate with the smallest tuple (cost, |dy| + |dx|, dy, dx) in lexicographic order, dy and dx compared as signed
 *                integers: among equal costs the zero vector wins, then the shortest vector in L1, then the one furthest up, then the
 *                one furthest left.  The rule does not depend on the order in which candidates are evaluated: the same call gives the
 *                same bits every time.  (R <= 15 lets the tuple pack into 31 bits -- 16 of cost, 5 of L1, 5 of dy + R, 5 of dx + R.)
 *   Sign.        block (r, c) of a looks like b at (y0 + dy, x0 + dx): with b the earlier picture, that is where the block came from.
 *   Record.      per block int32_t [4] = { dy, dx, cost, cost_zero }, cost_zero = cost(0, 0); 16 bytes, written exactly once.  The
 *                field of a picture is int32_t [rows][cols][4], row-major and dense.  The sum of cost_zero over the field is the Y sad
 *                of hvq_picture_metrics for the same pair when B tiles the picture.
 * hvq_motion_blocks (host only) returns rows * cols of a width x height picture and fills dims = { rows, cols } (dims may be NULL):
 *   HVQ_E_GEOMETRY for a geometry hvq_stream_open refuses, HVQ_E_ARG for a block other than 8 or 16 and for B = 16 on a picture that is
 *   not a multiple of 16 in both directions.
 * hvq_picture_motion:
 *   out[i]: a non-null DEVICE pointer, a multiple of 16, to the field of picture i (16 * hvq_motion_blocks bytes); every record of it is
 *       written whatever was there before (no memset, no atomics); nothing outside it is written.
 *   a_i = the resident picture (streams[i], ordinals[i]).  ref: HvqMetricsRef, its two non-trivial forms as for hvq_picture_ssim:
 *       stream >= 0 -- a resident picture of the same width, height and sampling, of any stream, ptr NULL; stream == -1 with ptr -- the
 *       caller's device memory in slot layout (Y first), a multiple of 16.  Motion against zeros means nothing: ref == NULL (with n > 0)
 *       and an entry { -1, *, NULL } are HVQ_E_ARG.
 *   Lookup, HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain and slot safety are hvq_picture_metrics'; the
 *   batch in flight is ended only when a requested picture (a or b) belongs to it.  HVQ_E_ARG for a NULL context, a block other than 8 or
 *   16, B = 16 on a stream it does not tile, a radius outside [0, HVQ_MOTION_MAX_RADIUS], a bad stream or ordinal, the refusals of `ref`
 *   above and of hvq_picture_metrics, a null `out`, an out[i] that is null or not a multiple of 16, n above 65535.  n == 0 is HVQ_OK and
 *   does nothing.  Every argument is checked before anything is enqueued: a refused call enqueues nothing and leaves every field
 *   untouched.  HVQ_E_NOGPU (after those checks) from a build without the motion kernel. */
#define HVQ_MOTION_MAX_RADIUS 15
int  hvq_motion_blocks(int width, int height, int h_samp, int v_samp, int block, int32_t dims[2]);
int  hvq_picture_motion(HvqContext *ctx, int n, const int *streams, const int *ordinals, const HvqMetricsRef *ref,
                        int block, int radius, int32_t *const *out, void *hip_stream);

/* Baseline JPEG (JFIF) files of resident pictures, written where the pictures lie: for `n` pictures, of any streams, sizes and samplings,
 * each becomes one complete file in the caller's DEVICE memory, on the caller's HIP stream and without a host synchronisation; the file
 * lengths are left in device memory.  The codec's display arithmetic is JFIF's full-range Y / Cb / Cr and its samplings are JPEG's, so a
 * file needs no colour conversion and no resampling and decodes to what the player shows.  The bytes are specified exactly:
 *   Geometry.    W x H luma samples (multiples of 8), chroma planes (W / h_samp) x (H / v_samp).  An MCU is 8 h_samp x 8 v_samp luma samples;
 *                mw = ceil(W / (8 h_samp)), mh = ceil(H / (8 v_samp)).  Every plane is extended to whole blocks by repeating its last column,
 *                then its last row.  Blocks of an MCU: the Y blocks in raster order (v_samp rows of h_samp), then Cb (= U), then Cr (= V).
 *   Transform.   Integers only.  x = sample - 128.  C[k][n] = floor(s_k cos((2 n + 1) k pi / 16) 8192 + 0.5), s_0 = sqrt(1 / 8), s_k = 1 / 2
 *                otherwise, for n < 4; C[k][7 - n] = C[k][n] for even k, -C[k][n] for odd k.  Rows k = 0 .. 7, n = 0 .. 3:
 *                    2896 2896 2896 2896 / 4017 3406 2276 799 / 3784 1567 -1567 -3784 / 3406 -799 -4017 -2276 /
 *                    2896 -2896 -2896 2896 / 2276 -4017 799 3406 / 1567 -3784 3784 -1567 / 799 -2276 3406 -4017
 *                Rows first: r[y][k] = (sum_n C[k][n] x[y][n] + 1024) >> 11; then columns: F[k][l] = (sum_y C[k][y] r[y][l] + 16384) >> 15,
 *                both shifts arithmetic.  The sums are exact in 32 bits (below 2^23 and 2^27).  Any evaluation order or even/odd
 *                factorisation that yields the same integers is allowed; no other intermediate rounding is.
 *   Range.       With A = sum |C[k][y] C[l][n]| <= 23168^2 (rows 0 and 4 have the largest absolute sum, 8 x 2896): an AC basis has as much
 *                positive as negative weight (every row k > 0 sums to 0), samples lie in [-128, 127], so the unrounded AC value is at most
 *                255 A / 2 / 2^26 < 1019.9; the row rounding adds at most 23168 / 2 / 2^15 < 0.36 and the last rounding 0.5: |AC| <= 1020.
 *                The unrounded DC lies in [-128, 127] A / 2^26 = [-1023.8, 1015.8]: -1024 <= DC <= 1016, differences below 2048.  So AC
 *                sizes never exceed 10 and DC difference sizes never exceed 11: what the tables below code.
 *   Quantising.  Base tables: ITU-T T.81 Annex K.1 (luminance) and K.2 (chrominance).  Quality q in 1 .. 100 scales them as the IJG
 *                library does: s = 5000 / q (integer division) for q < 50, else 200 - 2 q; Q[i] = clamp((base[i] s + 50) / 100, 1, 255).
 *                Coefficient = sign(F) ((|F| + (Q >> 1)) / Q), integer division.
 *   Coding.      Baseline Huffman with the tables of Annex K.3 - K.6 (K.3 / K.5 for Y, K.4 / K.6 for Cb and Cr), zigzag order, DC
 *                differences per component, (run, size) symbols, ZRL = 0xF0, EOB = 0x00 unless coefficient 63 is non-zero; a negative
 *                value v of size s is written as v + 2^s - 1.  Restart interval = one MCU row (Ri = mw): every interval starts with the
 *                three DC predictors at 0 and is padded with 1-bits to a byte; inside entropy data every 0xFF is followed by 0x00; interval
 *                j < mh - 1 is followed by the marker FF D0 + (j mod 8).  Every MCU row is thus an independent, byte-aligned piece.
 *   Segments.    In this order, HVQ_JPEG_HEADER (629) bytes up to the entropy data for every geometry and quality: SOI; APP0 "JFIF\0",
 *                version 1.01, units 0, density 1 x 1, no thumbnail; DQT table 0 (8-bit, zigzag order); DQT table 1; SOF0, precision 8, H,
 *                W, 3 components: id 1 sampling h_samp << 4 | v_samp table 0, id 2 0x11 table 1, id 3 0x11 table 1; DHT DC0, DHT AC0, DHT
 *                DC1, DHT AC1, one segment each; DRI = mw; SOS, 3 components, table selectors 0x00 / 0x11 / 0x11, Ss 0, Se 63, Ah / Al 0;
 *                the entropy data; EOI.
 * hvq_jpeg_header (host only) writes those HVQ_JPEG_HEADER bytes to dst (cap bytes) and their count to *len (len may be NULL):
 *   HVQ_E_GEOMETRY for a geometry hvq_stream_open refuses, HVQ_E_ARG for a quality outside 1 .. 100, a null dst or a cap below the count.
 * hvq_jpeg_bound (host only): a length no file of this geometry exceeds at any quality, 0 for a refused geometry:
 *   629 + 2 + 2 (mh - 1) + 2 mh ceil(mw (h_samp v_samp + 2) 64 x 26 / 8) -- header, EOI, the RST markers, and per interval its blocks at 26
 *   bits a coefficient (the longest AC code, 16, with 10 value bits; a DC difference takes 11 + 11 at most; a ZRL stands for 16
 *   coefficients in 11 bits), rounded up to a byte, every byte stuffed.
 * hvq_encode_jpeg:
 *   a_i = the resident picture (streams[i], ordinals[i]); with src != NULL, src[i] != NULL and ordinals[i] == -1 it is the caller's device
 *       memory in slot layout (Y | U | V of stream streams[i]'s geometry, a multiple of 16), exactly as hvq_picture_checksums' src.
 *   out[i]: a non-null DEVICE pointer, a multiple of 16, with cap[i] bytes (cap: host memory).  The file starts at out[i]; nothing at or
 *       beyond out[i] + cap[i] is ever written.
 *   lengths: a DEVICE pointer, a multiple of 8, to n values.  lengths[i] is always written and is the length of the complete file,
 *       whether or not it fitted.  When lengths[i] <= cap[i] the bytes [0, lengths[i]) are the file, each written once, and the bytes
 *       after them are untouched.  When it is larger the contents of out[i] within cap[i] are unspecified (this build writes none): call
 *       again with more room.
 *   Lookup, HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain and slot safety are hvq_picture_metrics'; the
 *   batch in flight is ended only when a requested picture belongs to it.  HVQ_E_ARG for a NULL context, a quality outside 1 .. 100, a
 *   bad stream or ordinal, a null `out`, `cap` or `lengths`, an out[i] that is null or not a multiple of 16, a `lengths` that is not a
 *   multiple of 8, a cap[i] below HVQ_JPEG_HEADER + 2, a src[i] with an ordinal other than -1 or not a multiple of 16, n above 65535.
 *   n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is enqueued: a refused call enqueues nothing and
 *   leaves every destination and `lengths` untouched.  HVQ_E_NOGPU (after those checks) from a build without the JPEG kernels. */
#define HVQ_JPEG_HEADER 629
int    hvq_jpeg_header(int width, int height, int h_samp, int v_samp, int quality, uint8_t *dst, size_t cap, size_t *len);
size_t hvq_jpeg_bound(int width, int height, int h_samp, int v_samp);
int    hvq_encode_jpeg(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src, int quality,
                       void *const *out, const uint64_t *cap, uint64_t *lengths, void *hip_stream);

/* Perceptual hashes of resident pictures, computed where they lie: for `n` pictures, of any streams, sizes and samplings, in one kernel
 * launch and a small finishing launch behind it, on the caller's HIP stream and without a host synchronisation, three 64-bit hashes of
 * the luma plane.  "Have I seen this picture before?" is then a matter of Hamming distances between 8-byte values (hvq_hash_nearest);
 * no picture moves.  The values are specified as exact integers: this text is the authority for them.  It is a construction of the same
 * kind as the well-known aHash, dHash and pHash and makes no claim to equal the output of any library (those shrink pictures with float
 * filters).
 *   Plane.       Everything works on the luma plane only: a[y][x], W x H samples of 8 bits, W and H multiples of 8 up to 8192 (what
 *                hvq_stream_open accepts).  Chroma and sampling only matter for locating plane Y in the slot.
 *   Area grids.  A grid of gy rows x gx columns divides the plane into equal rectangles with rational edges.  In integers:
 *                wy(r, y) = max(0, min(gy y + gy, H r + H) - max(gy y, H r)) for 0 <= r < gy, 0 <= y < H; wx(c, x) the same with gx and W.
 *                Cell sum S[r][c] = sum over y, x of wy(r, y) wx(c, x) a[y][x].  Every cell has total weight W H (sum_r wy = gy,
 *                sum_y wy(r, y) = H); S <= 255 W H < 2^34: a cell is a 64-bit integer (a 32-bit cell is wrong from W H = 16 843 010
 *                samples on).  Nothing is rounded.  A plane narrower or lower than the grid spreads a sample over several cells; the
 *                formula is unchanged.  Three grids are used: S32 (32 x 32), S8 (8 x 8) and D (8 rows x 9 columns).  Two identities
 *                hold, and an implementation may rely on them: 16 S8[r][c] = the sum of the 4 x 4 block of S32 at (4 r, 4 c);
 *                4 D[r][c] = the sum of rows 4 r .. 4 r + 3 of the 32-row x 9-column grid.
 *   Bit order.   A hash is 64 bits taken row-major from an 8 x 8 array of booleans: element (r, c) is bit 63 - (8 r + c).  Printed as 16 hex
 *                digits it reads left to right, top to bottom.
 *   aHash.       T = sum of all S8 (= 64 sum a).  bit(r, c) = 64 S8[r][c] > T.
 *   dHash.       bit(r, c) = D[r][c + 1] > D[r][c], 0 <= c < 8.
 *   pHash.       m[r][c] = (16 S32[r][c] + (W H >> 1)) / (W H), integer division: the cell mean in sixteenths, 0 .. 4080.
 *                F[k][l] = sum over r, c of C[k][r] C[l][c] m[r][c] for 0 <= k, l < 8, exact, |F| < 2^46 (the pass over c fits 32 bits,
 *                the pass over r needs 64).  Sort the 64 values, f_0 <= ... <= f_63: bit(k, l) = 2 F[k][l] > f_31 + f_32 -- "above the
 *                median", the even-count median without its division.
 *                C[k][n] = floor(4096 cos((2 n + 1) k pi / 64) + 0.5): the unnormalised DCT-II.  C[0][n] = 4096 and
 *                C[k][31 - n] = (-1)^k C[k][n].  The table is committed as constants (hvq_phash.h); rows k = 1 .. 7, n = 0 .. 15:
 *                    4091 4052 3973 3857 3703 3513 3290 3035 2751 2440 2106 1751 1380 995 601 201
 *                    4076 3920 3612 3166 2598 1931 1189 401 -401 -1189 -1931 -2598 -3166 -3612 -3920 -4076
 *                    4052 3703 3035 2106 995 -201 -1380 -2440 -3290 -3857 -4091 -3973 -3513 -2751 -1751 -601
 *                    4017 3406 2276 799 -799 -2276 -3406 -4017 -4017 -3406 -2276 -799 799 2276 3406 4017
 *                    3973 3035 1380 -601 -2440 -3703 -4091 -3513 -2106 -201 1751 3290 4052 3857 2751 995
 *                    3920 2598 401 -1931 -3612 -4076 -3166 -1189 1189 3166 4076 3612 1931 -401 -2598 -3920
 *                    3857 2106 -601 -3035 -4091 -3290 -995 1751 3703 3973 2440 -201 -2751 -4052 -3513 -1380
 *                No entry is within 0.02 of a rounding tie.  Every row k > 0 sums to exactly 0: a constant added to the picture changes
 *                only F[0][0].
 *   Known answers.  A flat picture of value v > 0, any size: { 0, 0, 0x8000000000000000, v W H }; of value 0: { 0, 0, 0, 0 } (all F are
 *                0, none is above the median).  64 x 64 with columns 0 .. 31 = 255 and the rest 0: ahash 0xF0F0F0F0F0F0F0F0, dhash 0; its
 *                mirror: ahash 0x0F0F0F0F0F0F0F0F, dhash 0x1818181818181818 (column 4 of the 9-column grid is half covered).  ahash
 *                and dhash are invariant under a + c without clipping; phash too while F[0][0] stays above f_32.
 *   out: `n` records of uint64_t [4] = { ahash, dhash, phash, sum_y } (HVQ_HASH_*), 32 bytes each, dense, in call order, in DEVICE memory, a
 *       multiple of 8.  sum_y = T / 64, the plain sum of the luma samples (sum_a of plane Y of hvq_picture_metrics).  The call writes all
 *       32 n bytes whatever they held before.  All sums are integer sums: the record does not depend on the order the GPU adds in.
 *   a_i, `src`, lookup, HVQ_E_STATE and HVQ_E_ARG cases, n <= 65535, ordering on `hip_stream`, membership of the export chain, slot safety
 *   and ending the batch in flight only when a requested picture belongs to it are hvq_picture_checksums', word for word.  n == 0 is
 *   HVQ_OK and does nothing.  Every argument is checked before anything is enqueued: a refused call leaves `out` untouched.  HVQ_E_NOGPU
 *   (after those checks) from a build without the hash kernels. */
#define HVQ_HASH_AHASH 0
#define HVQ_HASH_DHASH 1
#define HVQ_HASH_PHASH 2
#define HVQ_HASH_SUM_Y 3
int  hvq_picture_hashes(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src, uint64_t *out,
                        void *hip_stream);

/* Nearest hashes by Hamming distance, on hashes that lie in DEVICE memory: one launch on `hip_stream`, no host synchronisation.
 *   q, db: device pointers, multiples of 8.  Query i is q[i * q_stride], candidate j is db[j * db_stride]; the strides count uint64_t and
 *       are at least 1 (a stride of 4 walks one column of hvq_picture_hashes' records).  q and db may overlap or be equal.
 *   d(i, j) = popcount(q_i ^ db_j).  The candidates of query i are all 0 <= j < ndb when self_offset < 0, otherwise those with
 *       j < self_offset + i ("earlier than me": q == db with offset 0 is de-duplication in place; a block of queries starting at k uses
 *       offset k).
 *   out: `nq` records of int32_t [4] = { nearest, distance, within, first_within } (HVQ_NEAR_*), 16 bytes each, dense, in DEVICE memory, a
 *       multiple of 16.  nearest is the candidate with the smallest (d, j), distance its d; within is the number of candidates with
 *       d <= threshold, first_within the smallest such j or -1.  A query without candidates has { -1, 65, 0, -1 }.  Every record is
 *       written exactly once (one 16-byte store) and does not depend on the order of evaluation.
 *   0 <= threshold <= 64; 0 <= nq, ndb <= HVQ_HASH_NEAREST_MAX (2^24).  nq == 0 does nothing; ndb == 0 writes the empty records.
 *   The call reads no resident picture and is no member of the export chain: it is just a launch on `hip_stream`, ordered by that
 *   stream behind the work that produced the hashes.  HVQ_E_ARG for a NULL context, a NULL or misaligned q, db (with ndb > 0) or out, a
 *   stride below 1, a threshold outside 0 .. 64, a count out of range; a refused call leaves `out` untouched.  HVQ_E_NOGPU (after those
 *   checks) from a build without the hash kernels. */
#define HVQ_NEAR_NEAREST 0
#define HVQ_NEAR_DISTANCE 1
#define HVQ_NEAR_WITHIN 2
#define HVQ_NEAR_FIRST_WITHIN 3
#define HVQ_HASH_NEAREST_MAX (1 << 24)
int  hvq_hash_nearest(HvqContext *ctx, const uint64_t *q, int nq, int q_stride, const uint64_t *db, int ndb, int db_stride,
                      int64_t self_offset, int threshold, int32_t *out, void *hip_stream);

/* Resident pictures resampled into uint8 pictures of ANOTHER geometry in slot layout, where they lie: for `n` pictures, of any streams,
 * sizes and samplings, in one kernel launch on the caller's HIP stream and without a host synchronisation, each picture's three planes
 * through the area (box) filter with rational cell edges -- the construction of hvq_picture_hashes' grids -- into DEVICE memory laid
 * out as a slot of the target geometry is.  Whatever takes "the caller's device memory in slot layout" (`src` of hvq_picture_checksums,
 * hvq_picture_histograms, hvq_encode_jpeg, hvq_picture_hashes; `ref.ptr` of hvq_picture_metrics, hvq_picture_ssim, hvq_picture_motion)
 * takes the result, given an open stream of the target geometry to carry it (nothing need ever be submitted to that stream).  The values
 * are specified as exact integers: this text is the authority for them.
 *   Planes.    Each of the three planes is resampled on its own.  The source plane is the crop's part of plane p, Ny rows x Nx samples:
 *              for Y the crop itself, for U and V the crop's edges divided by the SOURCE sampling.  The target plane has My x Mx
 *              samples, from the target geometry; its sampling may differ from the source's (4:4:4 -> 4:2:0, 4:2:2 -> 4:2:0 and the
 *              reverse): chroma is simply another plane with its own N and M.
 *   Values.    wy(r, y) = max(0, min(My (y + 1), Ny (r + 1)) - max(My y, Ny r))   0 <= r < My, 0 <= y < Ny   (sum over y = Ny)
 *              wx(c, x) likewise with Mx, Nx
 *              S[r][c]  = sum over y, x of wy(r, y) wx(c, x) a[y][x]              exact; S <= 255 Nx Ny < 2^34: 64 bits
 *              D        = Nx Ny
 *              out[r][c] = (S[r][c] + (D >> 1)) / D                               integer division: round half up, ONE rounding
 *              Any evaluation order, separable or not, that yields these integers is allowed; no intermediate rounding is.  The
 *              horizontal partial sums (sum over x of wx a) fit 21 bits.  32-bit cells serve a plane only when 255 Nx Ny < 2^32
 *              (hvq_picture_hashes' threshold); beyond it a cell is 64 bits.
 *   Known answers.  M == N is the identity.  An integer reduction k is the k x k box mean rounded half up: the 2 x 2 block {0, 0, 0, 2}
 *              gives 1 and {0, 0, 0, 1} gives 0.  An integer enlargement replicates samples.  A flat picture stays flat at any ratio.
 *   dst[i]:    ptr: a non-null DEVICE pointer, a multiple of 16: Y | U | V tightly packed, the target geometry's slot layout,
 *              hvq_scale_bytes(width, height, h_samp, v_samp) bytes.  Exactly those bytes are written, each once and whatever was there
 *              before; nothing outside them is written (no memset, no atomics on the output).
 *              width, height, h_samp, v_samp: the target geometry, one that hvq_stream_open accepts (else HVQ_E_GEOMETRY).
 *              crop_x, crop_y, crop_w, crop_h: the source crop in luma samples; crop_w == 0 (then all four are 0): the whole picture.
 *   hvq_scale_bytes (host only): bytes of a picture of that geometry, or HVQ_E_GEOMETRY.
 *   hvq_scale_body (host only): the body of the kernel a plane of nx x ny samples takes on its way to mx x my: HVQ_SCALE_DIRECT (no
 *              sample has more than 2 x 2 taps: identity and enlargement) or HVQ_SCALE_TILED (the source rows of a tile of targets go
 *              through LDS, horizontal sums once, then the vertical pass); HVQ_E_ARG beyond the limits below.  The values do not depend
 *              on it.  hvq_scale_force_direct(ctx, 1) makes every later call of the context take the direct body (0: the chosen one
 *              again) and returns the setting before: for tests that compare the two with ==.
 *   HVQ_E_ARG for the whole call: for any plane and axis N > 32 M (a reduction beyond 32 is refused rather than done badly;
 *              enlargement is unlimited, it has at most two taps per axis); a crop that is empty or leaves the picture; a crop whose x
 *              values are no multiples of the source h_samp or whose y values are no multiples of the source v_samp; a cropped source
 *              narrower or lower than 8 luma samples; a null or misaligned ptr; n above 65535; a bad stream or ordinal; a src[i] with an
 *              ordinal other than -1 or that is no multiple of 16; a NULL context.  n == 0 is HVQ_OK and does nothing.  Every
 *              argument is checked before anything is enqueued: a refused call leaves every destination untouched.  HVQ_E_NOGPU (after
 *              those checks) from a build without the scale kernel.
 *   a_i and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_picture_metrics'. */
typedef struct HvqScaleDst {
    void   *ptr;                                  /* device, multiple of 16: Y | U | V tightly packed, the target geometry's slot layout */
    int32_t width, height, h_samp, v_samp;        /* target geometry: one that hvq_stream_open accepts */
    int32_t crop_x, crop_y, crop_w, crop_h;       /* source crop in luma samples; crop_w == 0 (all four 0): the whole picture */
} HvqScaleDst;
#define HVQ_SCALE_DIRECT 0
#define HVQ_SCALE_TILED  1
#define HVQ_SCALE_MAX_RATIO 32
int     hvq_scale_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                           const HvqScaleDst *dst, void *hip_stream);
int64_t hvq_scale_bytes(int width, int height, int h_samp, int v_samp);
int     hvq_scale_body(int nx, int ny, int mx, int my);
int     hvq_scale_force_direct(HvqContext *ctx, int on);

/* Resident pictures FILTERED into uint8 pictures of THEIR OWN geometry in slot layout, where they lie: for `n` pictures, of any streams,
 * sizes and samplings, in one kernel launch on the caller's HIP stream and without a host synchronisation, each plane through a sum of
 * up to two separable integer kernels with one rounding.  Gaussian and binomial blur, Sobel / Scharr gradients and their magnitude,
 * the Laplacian, a difference of Gaussians and unsharp masking are parameter sets of it (hvqm4_amd.filters builds them).  The result
 * composes like hvq_scale_pictures': whatever takes `src` or `ref.ptr` takes it.  The values are specified as exact integers: this
 * text is the authority for them.
 *   Planes.    Y is filtered with filter.luma, U and V with filter.chroma, each at its own resolution: Ny rows x Nx samples a.
 *   Values.    cx(v) = min(max(v, 0), Nx - 1), cy likewise: the border replicates the edge sample.  For term t of the plane's filter
 *              T_t[y][x] = sum over j in [0, 2 ry_t], i in [0, 2 rx_t] of wy_t[j] wx_t[i] a[cy(y + j - ry_t)][cx(x + i - rx_t)]
 *              -- correlation: tap i meets the sample i - rx to the right, nothing is flipped.  With terms == 1, T_1 = 0.
 *              S   = T_0 + T_1 (HVQ_FLT_SUM), |T_0 + T_1| (HVQ_FLT_ABS_SUM) or |T_0| + |T_1| (HVQ_FLT_SUM_ABS)
 *              h   = shift ? 1 << (shift - 1) : 0
 *              out = min(255, max(0, floor((S + h) / 2^shift) + bias))
 *              The floor is towards minus infinity (an arithmetic shift): ONE rounding, half up, for negative sums too: S = -1,
 *              shift = 1 gives 0 and S = -3, shift = 1 gives -1.  Any evaluation order that yields these integers is allowed; no
 *              intermediate rounding is.  With gain = sum over t of (sum |wx_t|) (sum |wy_t|) <= HVQ_FLT_MAX_GAIN = 2^22, every
 *              partial sum and |S| + h stay below 255 * 2^22 + 2^21 < 2^31: 32-bit signed arithmetic serves everywhere.
 *   Known answers.  The identity (terms 1, radii 0, weights {1}, shift 0, bias 0) copies the plane.  wx = {1, 0, 0} with rx = 1 (wy =
 *              {1}) gives out[x] = a[max(x - 1, 0)]: orientation and border.  A flat plane stays flat whenever the weights sum to
 *              2^shift.  {1, 2, 1} x {1, 2, 1}, shift 4, on the 3 x 3 plane that is 0 but for a 16 in the middle gives {1, 2, 1; 2, 4, 2;
 *              1, 2, 1}.  Sobel-x ({-1, 0, 1} x {1, 2, 1}) with bias 128 on a flat plane gives 128.  The two negative ties above.
 *   hvq_filter_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL filter or, in either plane: terms other than 1 or 2; a radius outside
 *              0 .. HVQ_FLT_MAX_RADIUS; a tap beyond the first 2 r + 1 that is not 0 (of a term in use); combine outside the three
 *              values; shift outside 0 .. HVQ_FLT_MAX_SHIFT; bias outside -255 .. 255; a gain of 0 or above HVQ_FLT_MAX_GAIN.
 *              A term that is not in use (term[1] with terms == 1) is not looked at.
 *   The call.  Output i has the geometry of its source, in slot layout (Y | U | V tightly packed): dst[i] is a non-null DEVICE pointer,
 *              a multiple of 16, of hvq_stream_pic_bytes bytes.  Exactly those bytes are written, each once and whatever was there
 *              before; nothing outside them is written (no memset, no atomics).  dst[i] must not overlap any source of the call: the
 *              caller's business, not checked.  which[i] selects filters[which[i]]; which == NULL: filters[0] for all.  nfilters is
 *              1 .. HVQ_FLT_MAX_FILTERS; every filter of the table is checked, used or not.
 *              hvq_filter_force_filter(ctx, 1) makes every later call of the context run identity planes through the filter body
 *              instead of the copy body (0: the chosen one again) and returns the setting before: for tests that compare the two with ==.
 *   HVQ_E_ARG for the whole call: what hvq_filter_check refuses; nfilters outside 1 .. 64; a which[i] outside 0 .. nfilters - 1; a null
 *              or misaligned dst[i]; n above 65535; a bad stream or ordinal; a src[i] with an ordinal other than -1 or that is no
 *              multiple of 16; a NULL context, filters or dst.  n == 0 is HVQ_OK and does nothing.  Every argument is checked before
 *              anything is enqueued: a refused call leaves every destination untouched.  HVQ_E_NOGPU (after those checks) from a build
 *              without the filter kernel.
 *   a_i and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_scale_pictures'. */
#define HVQ_FLT_MAX_RADIUS 15
#define HVQ_FLT_MAX_TAPS   31            /* 2 * radius + 1 */
#define HVQ_FLT_MAX_SHIFT  22
#define HVQ_FLT_MAX_GAIN   (1 << 22)
#define HVQ_FLT_MAX_FILTERS 64
#define HVQ_FLT_SUM      0               /* S = T0 + T1          */
#define HVQ_FLT_ABS_SUM  1               /* S = |T0 + T1|        */
#define HVQ_FLT_SUM_ABS  2               /* S = |T0| + |T1|      */
typedef struct HvqFilterTerm  { int32_t rx, ry; int16_t wx[HVQ_FLT_MAX_TAPS], wy[HVQ_FLT_MAX_TAPS]; } HvqFilterTerm;
typedef struct HvqPlaneFilter { int32_t terms, combine, shift, bias; HvqFilterTerm term[2]; } HvqPlaneFilter;
typedef struct HvqFilter      { HvqPlaneFilter luma, chroma; } HvqFilter;   /* chroma serves U and V, at their own resolution */
int     hvq_filter_check(const HvqFilter *f);
int     hvq_filter_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                            const HvqFilter *filters, int nfilters, const int *which, void *const *dst, void *hip_stream);
int     hvq_filter_force_filter(HvqContext *ctx, int on);

/* Resident pictures WARPED into uint8 pictures of a TARGET GEOMETRY in slot layout, where they lie: for `n` pictures, of any streams,
 * sizes and samplings, in one kernel launch on the caller's HIP stream and without a host synchronisation, each plane through its own
 * affine inverse map with bilinear taps in exact integers and one rounding.  Translation (stabilising a clip by its global motion),
 * the mirrors, the transpose, the quarter turns (a portrait clip turned upright: the target swaps width and height), rotation, zoom
 * and shear are parameter sets of it (hvqm4_amd.warp builds them); warp plus resize is one call.  The result composes like
 * hvq_scale_pictures': whatever takes `src` or `ref.ptr` takes it.  The values are specified as exact integers: this text is the
 * authority for them.
 *   The map.   warps[i] = { m00, m01, m10, m11, t0, t1 } in Q16 (65536 = 1.0) maps TARGET luma coordinates to SOURCE luma coordinates:
 *              u = m00 x + m01 y + t0, v = m10 x + m11 y + t1.  Sample centres lie at integer + 1/2; chroma is sited at the centre of
 *              its luma cell (what the area filter of hvq_scale_pictures implies).
 *   Values.    Plane p has target sampling (hx', vy') and source sampling (hx, vy), both (1, 1) for Y; the target plane has My x Mx
 *              samples, the source plane a has Ny x Nx.  For target sample (x, y):
 *              NU = m00 hx' (2x + 1) + m01 vy' (2y + 1) + 2 t0 - 65536 hx          (64 bits; Q17 luma units)
 *              NV = m10 hx' (2x + 1) + m11 vy' (2y + 1) + 2 t1 - 65536 vy
 *              U8 = floor((NU + 256 hx) / (512 hx))     V8 = floor((NV + 256 vy) / (512 vy))     (arithmetic shifts: hx, vy are 1 or 2)
 *              ix = floor(U8 / 256), fx = U8 - 256 ix (0 .. 255); iy, fy likewise
 *              tap(j, i) = a[cy(iy + j)][cx(ix + i)]                        border == HVQ_WARP_REPLICATE (cx, cy clamp into the plane)
 *                        = inside the plane ? a[iy + j][ix + i] : fill[p]   border == HVQ_WARP_CONSTANT
 *              S   = (256 - fy) ((256 - fx) tap(0,0) + fx tap(0,1)) + fy ((256 - fx) tap(1,0) + fx tap(1,1))
 *              out = (S + 32768) >> 16                                      ONE rounding; S + 32768 < 2^31
 *              Any evaluation order that yields these integers is allowed; no intermediate rounding is.  Saturating U8 to
 *              [-512, 256 Nx] and V8 to [-512, 256 Ny] changes no value under either border (beyond them every tap lies on the same
 *              side outside the plane): behind it a lane works in 32 bits.  Inside a tile of 64 x 16 targets the deltas of NU and NV
 *              against the tile's first target stay below 2^31 under the limit on the coefficients.
 *   Limits.    |m..| <= HVQ_WARP_MAX_SCALE = 32 * 65536; t0, t1 any int32; border 0 or 1; pad 0.  A singular matrix is not refused: an
 *              all-zero linear part is a well-defined constant picture.
 *   Known answers.  The identity (m00 = m11 = 65536, the rest 0) copies every plane in every sampling.  t0 = 32768 gives
 *              (a[x] + a[x + 1] + 1) >> 1; m00 = 131072 gives (a[2x] + a[2x + 1] + 1) >> 1.  m00 = -65536, t0 = 65536 W is the exact
 *              mirror, in Y and in 2:1-sampled chroma alike; m00 = m11 = 0, m01 = m10 = 65536 the exact transpose; the three quarter
 *              turns are exact permutations whenever the chroma sampling is square.  A flat picture stays flat under REPLICATE.
 *   dst[i]:    ptr: a non-null DEVICE pointer, a multiple of 16: Y | U | V tightly packed, the target geometry's slot layout,
 *              hvq_scale_bytes(width, height, h_samp, v_samp) bytes.  Exactly those bytes are written, each once and whatever was there
 *              before; nothing outside them is written (no memset, no atomics).  It must not overlap a source of the call: the
 *              caller's business, not checked.  width, height, h_samp, v_samp: the target geometry, one that hvq_stream_open accepts
 *              (else HVQ_E_GEOMETRY).
 *   hvq_warp_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL record, a coefficient beyond the limit, a bad border, a non-zero pad.
 *   hvq_warp_body (host only): the body of the kernel a plane takes under a warp: (dst_h, dst_v) the TARGET sampling of the plane,
 *              (src_h, src_v) its SOURCE sampling (both 1, 1 for Y), nx x ny its source samples.  HVQ_WARP_DIRECT: every lane gathers
 *              its four taps from memory; serves every map.  HVQ_WARP_TILED: the source bounding box of a tile of 64 x 16 targets
 *              goes through LDS (the body for turns, where a row of targets crosses many source rows).  The values do not depend on
 *              it.  hvq_warp_force_direct(ctx, 1) makes every later call of the context take the direct body (0: the chosen one
 *              again; 2: the tiled one wherever LDS holds the box, for the measurement that sets the rule) and returns the setting
 *              before: for tests that compare the bodies with ==.
 *   HVQ_E_ARG for the whole call: what hvq_warp_check refuses; a null or misaligned ptr; n above 65535; a bad stream or ordinal; a
 *              src[i] with an ordinal other than -1 or that is no multiple of 16; a NULL context, warps or dst.  n == 0 is HVQ_OK and
 *              does nothing.  Every argument is checked before anything is enqueued: a refused call leaves every destination
 *              untouched.  HVQ_E_NOGPU (after those checks) from a build without the warp kernel.
 *   a_i and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_scale_pictures'. */
#define HVQ_WARP_MAX_SCALE (32 * 65536)
#define HVQ_WARP_REPLICATE 0
#define HVQ_WARP_CONSTANT  1
#define HVQ_WARP_DIRECT    0
#define HVQ_WARP_TILED     1
typedef struct HvqWarp {
    int32_t m00, m01, m10, m11, t0, t1;           /* Q16: target luma coordinates -> source luma coordinates */
    int32_t border;                               /* HVQ_WARP_REPLICATE or HVQ_WARP_CONSTANT */
    uint8_t fill[3];                              /* the value outside the plane under HVQ_WARP_CONSTANT: Y, U, V */
    uint8_t pad;                                  /* 0 */
} HvqWarp;
typedef struct HvqWarpDst {
    void   *ptr;                                  /* device, multiple of 16: Y | U | V tightly packed, the target geometry's slot layout */
    int32_t width, height, h_samp, v_samp;        /* target geometry: one that hvq_stream_open accepts */
} HvqWarpDst;
int     hvq_warp_check(const HvqWarp *w);
int     hvq_warp_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                          const HvqWarp *warps, const HvqWarpDst *dst, void *hip_stream);
int     hvq_warp_body(const HvqWarp *w, int dst_h, int dst_v, int src_h, int src_v, int nx, int ny);
int     hvq_warp_force_direct(HvqContext *ctx, int on);

/* Resident pictures COMPOSED into uint8 pictures of a TARGET GEOMETRY in slot layout: `ntargets` pictures, each built from an ordered
 * list of LAYERS -- rectangles of resident pictures (or of the caller's device memory), each with a signed integer weight per plane,
 * that replace (PUT) or join (ADD) what lies below them -- in one kernel launch on the caller's HIP stream and without a host
 * synchronisation.  Contact sheets, side-by-side and picture-in-picture, cross-fades and temporal averages, difference pictures and
 * translucent overlays are parameter sets of it (hvqm4_amd.compose builds them).  The result composes like hvq_scale_pictures':
 * whatever takes `src` or `ref.ptr` takes it.  The values are specified as exact integers: this text is the authority for them.
 *   Sources.   The sources of all layers are given flat, as every other call takes pictures: layer l reads picture (streams[l],
 *              ordinals[l]) or the caller's memory src[l] with ordinal -1; a picture used by several layers is repeated.  layers[l]
 *              holds the layer's numbers.  Target t takes layers[first .. first + count), in this order; ranges of several targets
 *              may share layers.  A layer's source has the sampling of every target that uses it.
 *   Values.    Plane p of a target has sampling (hx, vy), (1, 1) for Y.  A layer's rectangles in plane p are its luma numbers divided
 *              by hx (x numbers) and vy (y numbers), which they must be multiples of: sx_p, sy_p, w_p, h_p, dx_p, dy_p.  For target
 *              sample (x, y) of the plane, a_l the source of layer l:
 *              acc = 0
 *              for l in the target's layers, in order:
 *                  if dx_p <= x < dx_p + w_p and dy_p <= y < dy_p + h_p:
 *                      s   = a_l[p][y - dy_p + sy_p][x - dx_p + sx_p]
 *                      acc = (mode_l == HVQ_CMP_PUT ? 0 : acc) + weight_l[p] * s
 *              h   = shift ? 1 << (shift - 1) : 0
 *              out = min(255, max(0, floor((acc + h) / 2^shift) + bias[p]))
 *              The floor is towards minus infinity (an arithmetic shift): ONE rounding, half up, for negative sums too, the finish of
 *              hvq_filter_pictures.  Any evaluation order that yields these integers is allowed; no intermediate rounding is.  With
 *              gain_p = sum over the target's layers of |weight_l[p]| <= HVQ_CMP_MAX_GAIN = 2^22, |acc| + h stays below 255 * 2^22 +
 *              2^21 < 2^31: 32-bit signed arithmetic serves.  A sample that no layer covers is min(255, max(0, bias[p])): the
 *              background colour.
 *   Known answers.  One whole-picture PUT with weight 1 and shift 0 copies the picture, in every sampling.  Two ADDs of weight 1 with
 *              shift 1 give (a + b + 1) >> 1.  Weights +1 and -1 with bias 128 on equal pictures give 128 everywhere.  The two
 *              negative ties of the filter text: acc = -1, shift 1 gives 0 and acc = -3, shift 1 gives -1 (before the bias).  A PUT
 *              above ADDs discards them inside its rectangle only.  count == 0 is a flat picture of the bias.  A translucent overlay
 *              of alpha a / 256 over a region is PUT base (whole, 256), PUT base (region, 256 - a), ADD overlay (region, a), shift 8:
 *              (base (256 - a) + overlay a + 128) >> 8 inside the region with one rounding, base outside it.
 *   layers[l]: mode HVQ_CMP_PUT or HVQ_CMP_ADD.  sx, sy, w, h: the source rectangle in luma samples; w == 0 (then sx == sy == h == 0):
 *              the whole source.  dx, dy: where its top-left sample lands in the target, in luma samples.  weight[3]: Y, U, V.
 *   dst[t]:    ptr: a non-null DEVICE pointer, a multiple of 16: Y | U | V tightly packed, the target geometry's slot layout,
 *              hvq_scale_bytes(width, height, h_samp, v_samp) bytes.  Exactly those bytes are written, each once and whatever was there
 *              before; nothing outside them is written (no memset, no atomics).  It must not overlap a source of the call: the
 *              caller's business, not checked.  width, height, h_samp, v_samp: the target geometry, one that hvq_stream_open accepts
 *              (else HVQ_E_GEOMETRY).  first, count: its layers; count may be 0.  shift 0 .. HVQ_CMP_MAX_SHIFT; bias[3] -255 .. 255.
 *   hvq_compose_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL record, a mode outside the two values, a negative sx, sy, w, h, dx
 *              or dy, w == 0 with another of sx, sy, h not 0, or w > 0 with h == 0.
 *   Bodies.    A plane of a layer whose dx_p, w_p and sx_p - dx_p are all multiples of 4 takes the kernel's aligned body (one aligned
 *              source dword per target dword), any other the general body (a cover mask per byte, the bytes from the two aligned
 *              dwords that hold them).  The values do not depend on it.  hvq_compose_force_general(ctx, 1) makes every later call of
 *              the context take the general body everywhere (0: the chosen one again) and returns the setting before: for tests that
 *              compare the two with ==.
 *   HVQ_E_ARG for the whole call: what hvq_compose_check refuses; a layer of a target whose source sampling is not the target's (scale
 *              first); a source rectangle that leaves its source or a landing rectangle that leaves the target (nothing is clipped);
 *              x numbers that are no multiples of h_samp or y numbers that are no multiples of v_samp; a target's gain above
 *              HVQ_CMP_MAX_GAIN in a plane; shift or bias outside their ranges; first or count negative, first + count above nlayers,
 *              count above HVQ_CMP_MAX_LAYERS; ntargets above 65535 or nlayers above HVQ_CMP_MAX_TOTAL; a null or misaligned ptr; a
 *              bad stream or ordinal; a src[l] with an ordinal other than -1 or that is no multiple of 16; a NULL context, dst, or
 *              (with nlayers > 0) streams, ordinals or layers.  A layer that belongs to no target is checked like any other (against
 *              its source) but is not read.  ntargets == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is
 *              enqueued: a refused call leaves every destination untouched.  HVQ_E_NOGPU (after those checks) from a build without
 *              the compose kernel.
 *   a_l and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_scale_pictures'. */
#define HVQ_CMP_PUT 0                /* acc = w * s   : replaces what lies below, inside the layer's rectangle */
#define HVQ_CMP_ADD 1                /* acc += w * s                                                           */
#define HVQ_CMP_MAX_LAYERS 256       /* per target: a 16 x 16 contact sheet                                     */
#define HVQ_CMP_MAX_TOTAL  (1 << 18) /* layers per call                                                         */
#define HVQ_CMP_MAX_GAIN   (1 << 22) /* per target and plane: sum over its layers of |weight[p]|                */
#define HVQ_CMP_MAX_SHIFT  22
typedef struct HvqComposeLayer {
    int32_t mode;                                 /* HVQ_CMP_PUT or HVQ_CMP_ADD */
    int32_t sx, sy, w, h;                         /* source rectangle, luma samples; w == 0 (then sx == sy == h == 0): the whole source */
    int32_t dx, dy;                               /* where its top-left lands in the target, luma samples */
    int32_t weight[3];                            /* Y, U, V: signed integers */
} HvqComposeLayer;
typedef struct HvqComposeDst {
    void   *ptr;                                  /* device, multiple of 16: Y | U | V tightly packed, hvq_scale_bytes() bytes */
    int32_t width, height, h_samp, v_samp;        /* target geometry: one that hvq_stream_open accepts */
    int32_t first, count;                         /* its layers: layers[first .. first + count), in this order; count may be 0 */
    int32_t shift;                                /* 0 .. HVQ_CMP_MAX_SHIFT */
    int32_t bias[3];                              /* -255 .. 255 per plane */
} HvqComposeDst;
int     hvq_compose_check(const HvqComposeLayer *l);
int     hvq_compose_pictures(HvqContext *ctx, int nlayers, const int *streams, const int *ordinals, const void *const *src,
                             const HvqComposeLayer *layers, int ntargets, const HvqComposeDst *dst, void *hip_stream);
int     hvq_compose_force_general(HvqContext *ctx, int on);

/* Resident pictures through RANK FILTERS into uint8 pictures of THEIR OWN geometry in slot layout, where they lie: for `n` pictures, of
 * any streams, sizes and samplings, in one kernel launch on the caller's HIP stream and without a host synchronisation, each plane
 * through the minimum (erosion), the maximum (dilation), their difference (the range, a morphological gradient) or the median of a
 * rectangular window.  What hvq_filter_pictures cannot be: these select a sample, they are no sums.  Opening and closing are two calls
 * through `src` (hvqm4_amd.rank builds the steps).  The result composes like hvq_scale_pictures': whatever takes `src` or `ref.ptr`
 * takes it.  The values are exact by nature -- nothing is rounded -- and this text is the authority for them.
 *   Planes.    Y goes through rank.luma, U and V through rank.chroma, each at its own resolution: Ny rows x Nx samples a.
 *   Window.    cx(v) = min(max(v, 0), Nx - 1), cy likewise: the border replicates the edge sample (hvq_filter_pictures' clamps).
 *              W(y, x) is the multiset of the (2 ry + 1)(2 rx + 1) samples a[cy(y + j - ry)][cx(x + i - rx)], j in [0, 2 ry], i in
 *              [0, 2 rx]: a clamped coordinate counts as often as it occurs.
 *   Values.    HVQ_RNK_MIN: min W.  HVQ_RNK_MAX: max W.  HVQ_RNK_RANGE: max W - min W, which lies in 0 .. 255 and needs no clamp.
 *              HVQ_RNK_MEDIAN: the element of index (|W| - 1) / 2 of W sorted ascending.
 *   Limits.    MIN, MAX, RANGE: rx and ry each 0 .. HVQ_RNK_MAX_RADIUS, independently.  MEDIAN: rx == ry in {0, 1, 2}: 1 x 1, 3 x 3 or
 *              5 x 5.  pad is 0.
 *   Known answers.  Radius 0 copies the plane under MIN, MAX and MEDIAN and gives all zeros under RANGE.  A flat plane stays flat, and
 *              RANGE of a flat plane is 0.  A single 0 in a plane of 255 at (y, x) becomes under MIN exactly the rectangle [y - ry,
 *              y + ry] x [x - rx, x + rx] cut at the plane, of zeros; the same holds for a 255 in zeros under MAX.  MAX(a) == 255 -
 *              MIN(255 - a).  MEDIAN(255 - a) == 255 - MEDIAN(a).  A single outlier vanishes under MEDIAN 3 x 3.  MEDIAN 3 x 3 of {0, 0,
 *              0; 0, 255, 255; 255, 255, 255} at its centre is 255 (five of the nine).  At a corner of the plane the corner sample
 *              counts four times (3 x 3): {9, 1; 1, 1} has the median 1 at (0, 0) -- W = {9, 9, 9, 9, 1, 1, 1, 1, 1} -- and {9, 9; 1, 1}
 *              has 9 there.
 *   hvq_rank_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL record or, in either plane: an op outside the four values; a radius
 *              outside 0 .. HVQ_RNK_MAX_RADIUS; MEDIAN with rx != ry or a radius above 2; a pad that is not 0.
 *   The call.  Output i has the geometry of its source, in slot layout (Y | U | V tightly packed): dst[i] is a non-null DEVICE pointer,
 *              a multiple of 16, of hvq_stream_pic_bytes bytes.  Exactly those bytes are written, each once and whatever was there
 *              before; nothing outside them is written (no memset, no atomics).  dst[i] must not overlap any source of the call: the
 *              caller's business, not checked.  which[i] selects ranks[which[i]]; which == NULL: ranks[0] for all.  nranks is
 *              1 .. HVQ_RNK_MAX_RANKS; every entry of the table is checked, used or not.
 *   Bodies.    A plane that is copied (radius 0 under MIN, MAX or MEDIAN) takes the kernel's copy body, MIN / MAX / RANGE the min/max
 *              body (windows by doubling: its cost grows with the logarithm of the radius), MEDIAN 3 x 3 and 5 x 5 an exchange network
 *              each.  The values do not depend on it.  hvq_rank_force_general(ctx, 1) makes every later call of the context run the
 *              planes that are copied through the min/max body at radius 0 (0: the chosen one again) and returns the setting before:
 *              for tests that compare the two with ==.
 *   HVQ_E_ARG for the whole call: what hvq_rank_check refuses; nranks outside 1 .. 64; a which[i] outside 0 .. nranks - 1; a null or
 *              misaligned dst[i]; n above 65535; a bad stream or ordinal; a src[i] with an ordinal other than -1 or that is no multiple
 *              of 16; a NULL context, ranks or dst.  n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is
 *              enqueued: a refused call leaves every destination untouched.  HVQ_E_NOGPU (after those checks) from a build without
 *              the rank kernel.
 *   a_i and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_scale_pictures'. */
#define HVQ_RNK_MIN    0
#define HVQ_RNK_MAX    1
#define HVQ_RNK_RANGE  2
#define HVQ_RNK_MEDIAN 3
#define HVQ_RNK_MAX_RADIUS 15
#define HVQ_RNK_MAX_RANKS  64
typedef struct HvqRankPlane { int32_t op, rx, ry, pad; } HvqRankPlane;
typedef struct HvqRank      { HvqRankPlane luma, chroma; } HvqRank;          /* chroma serves U and V, at their own resolution */
int     hvq_rank_check(const HvqRank *r);
int     hvq_rank_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                          const HvqRank *ranks, int nranks, const int *which, void *const *dst, void *hip_stream);
int     hvq_rank_force_general(HvqContext *ctx, int on);

/* Resident pictures through BILATERAL FILTERS into uint8 pictures of THEIR OWN geometry in slot layout, where they lie: for `n` pictures,
 * of any streams, sizes and samplings, in one kernel launch on the caller's HIP stream and without a host synchronisation, each plane
 * through a weighted mean of a rectangular window whose weights depend on the samples themselves: smoothing that keeps edges.  The
 * sigma filter ("surface blur") and the joint / cross bilateral filter, whose weights come from another picture (the guide), are special
 * cases.  What hvq_filter_pictures cannot be: the weights are no constants and the filter is not separable.  hvqm4_amd.bilateral builds
 * the tables.  The result composes like hvq_scale_pictures': whatever takes `src` or `ref.ptr` takes it.  The values are exact
 * integers with one rounding, and this text is the authority for the bytes.
 *   Planes.    Y goes through bil.luma, U and V through bil.chroma, each at its own resolution: Ny rows x Nx samples a.  The guide plane g
 *              is the same plane of the guide picture, or a itself when the picture has no guide.
 *   Window.    cx(v) = min(max(v, 0), Nx - 1), cy likewise (hvq_rank_pictures' clamps): the border replicates the edge sample, and a
 *              clamped coordinate counts as often as it occurs.
 *   Weights.   For j in [-ry, ry] and i in [-rx, rx]: q = (cy(y + j), cx(x + i)), w(j, i) = spatial[|j|][|i|] * range[ |g[q] - g[y][x]| ].
 *              Both factors are uint8, so w <= 65025.
 *   Value.     den = sum w, num = sum w * a[q], out = (num + den / 2) / den: floor of the quotient, one rounding, half up.  No clamp is
 *              needed: a weighted mean of bytes is a byte.
 *   32 bits.   With radius 7 the window has 225 taps and the largest num + den / 2 is 225 * 65025 * 255 + 7315312 = 3738124687 < 2^32:
 *              every intermediate fits uint32.
 *   Limits.    rx, ry each 0 .. HVQ_BIL_MAX_RADIUS, independently.  spatial[0][0] >= 1 and range[0] >= 1: the centre tap then has a
 *              weight, so den >= 1 always.  pad is 0.  Entries of spatial outside [0, ry] x [0, rx] are not read.  A zero in spatial
 *              switches a tap off: a disc is a table with zero corners.
 *   Guide.     guide == NULL, or guide[i] == {-1, 0, NULL}: the picture guides itself.  Otherwise HvqMetricsRef's two non-trivial forms,
 *              with hvq_picture_metrics' checks and texts: stream >= 0 -- a resident picture of the source's geometry, no pointer; stream
 *              -1 with a pointer that is a multiple of 16 -- the caller's device memory in slot layout.  A guide of another geometry
 *              refuses the call.  A guide that belongs to the batch in flight ends that batch, as a source does.
 *   Known answers.  Radius 0 copies the plane.  A flat plane stays flat under any tables.  A range table with only range[0] != 0 copies the
 *              plane under any radius and spatial table.  range all ones and spatial all ones is the box mean with replicated borders,
 *              rounded half up.  {0, 1, 0} under spatial[0] = {2, 1}, ry = 0 and a flat range table gives 1 at its centre (2 / 4 rounds
 *              up).  A two-level step of 40 | 200 under range[d] = 0 for d >= 100 is left byte for byte as it is, at radius 7 with every
 *              other weight 255.  A flat guide makes the call a linear filter: with the spatial quadrant {4, 2; 2, 1} it is the 3 x 3
 *              binomial of hvq_filter_pictures exactly.  A picture guided by a copy of itself equals the unguided call.  Transposing the
 *              plane, the radii and spatial transposes the result; mirroring the plane mirrors it.
 *   hvq_bilateral_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL record or, in either plane: a radius outside 0 ..
 *              HVQ_BIL_MAX_RADIUS; spatial[0][0] == 0; range[0] == 0; a pad that is not 0.
 *   The call.  Output i has the geometry of its source, in slot layout (Y | U | V tightly packed): dst[i] is a non-null DEVICE pointer,
 *              a multiple of 16, of hvq_stream_pic_bytes bytes.  Exactly those bytes are written, each once and whatever was there
 *              before; nothing outside them is written (no memset, no atomics).  dst[i] must not overlap any source or guide of the
 *              call: the caller's business, not checked.  which[i] selects sets[which[i]]; which == NULL: sets[0] for all.  nsets is
 *              1 .. HVQ_BIL_MAX_SETS; every entry of the table is checked, used or not.
 *   Bodies.    A plane of radius 0 in both axes takes the kernel's copy body, every other the general one.  The values do not depend on
 *              it.  hvq_bilateral_force_general(ctx, 1) makes every later call of the context run the planes of radius 0 through the
 *              general body (0: the chosen one again) and returns the setting before: for tests that compare the two with ==.
 *   HVQ_E_ARG for the whole call: what hvq_bilateral_check refuses; nsets outside 1 .. 64; a which[i] outside 0 .. nsets - 1; a null or
 *              misaligned dst[i]; n above 65535; a bad stream or ordinal; a src[i] with an ordinal other than -1 or that is no multiple
 *              of 16; a guide with a stream and a pointer, of another geometry, of a stream below -1 or with a misaligned pointer; a NULL
 *              context, sets or dst.  n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is enqueued: a
 *              refused call leaves every destination untouched.  HVQ_E_NOGPU (after those checks) from a build without the bilateral
 *              kernel.
 *   a_i and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_scale_pictures'. */
#define HVQ_BIL_MAX_RADIUS 7
#define HVQ_BIL_MAX_SETS   64
typedef struct HvqBilateralPlane { int32_t rx, ry, pad[2]; uint8_t spatial[8][8]; uint8_t range[256]; } HvqBilateralPlane;  /* 336 bytes */
typedef struct HvqBilateral      { HvqBilateralPlane luma, chroma; } HvqBilateral;  /* chroma serves U and V, at their own resolution */
int     hvq_bilateral_check(const HvqBilateral *b);
int     hvq_bilateral_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                               const HvqMetricsRef *guide, const HvqBilateral *sets, int nsets, const int *which,
                               void *const *dst, void *hip_stream);
int     hvq_bilateral_force_general(HvqContext *ctx, int on);

/* Resident pictures through LOOKUP TABLES -- a point operation, out = table[in] -- into uint8 pictures of THEIR OWN geometry in slot
 * layout, where they lie: for `n` pictures, of any streams, sizes and samplings, in one kernel launch on the caller's HIP stream and
 * without a host synchronisation.  Equalisation, levels, gamma, inversion, posterising and binarisation are tables (hvqm4_amd.maps
 * builds them; hvq_histogram_tables below builds the ones that depend on the picture, on the GPU).  The result composes like
 * hvq_rank_pictures': whatever takes `src` or `ref.ptr` takes it.  This text is the authority for the bytes.
 *   Values.    Plane p (0 Y, 1 U, 2 V) of output i is T[p][a] for every sample a of plane p of the source, T = table which[i]: a record
 *              of uint8 [3][256], HVQ_MAP_TABLE_BYTES bytes.  Nothing is rounded.
 *   Known answers.  The identity table copies.  T[v] = 255 - v inverts.  Applying a table that is a permutation and then the table of
 *              its inverse permutation gives the source back.  A constant table gives a flat plane.
 *   Tables.    `tables` is a DEVICE pointer, a non-null multiple of 16: `ntables` records, dense.  They are read when the work runs on
 *              `hip_stream`, not at the call: an earlier launch on that stream may write them (hvq_histogram_tables).  ntables is
 *              1 .. 65535.  `which` is a HOST array: picture i takes record which[i].  which == NULL: ntables == 1 (every picture takes
 *              record 0) or ntables == n (picture i takes record i); anything else is HVQ_E_ARG.  Every byte value is a valid entry: the
 *              contents are not checked.
 *   planes.    A mask of the bits 0 .. 2 (Y, U, V).  A plane whose bit is clear is copied, not looked up (the kernel's copy body).  0 and
 *              values above 7 are HVQ_E_ARG.
 *   The call.  Output i has the geometry of its source, in slot layout (Y | U | V tightly packed): dst[i] is a non-null DEVICE pointer,
 *              a multiple of 16, of hvq_stream_pic_bytes bytes.  Exactly those bytes are written, each once and whatever was there
 *              before; nothing outside them is written (no memset, no atomics).  dst[i] MAY EQUAL src[i] exactly (in place on the
 *              caller's memory): a lane reads only the dwords that it later writes.  Any other overlap of a destination with a source
 *              or another destination is the caller's business, not checked.
 *   Kernel.    A tile is HVQ_MP_TILE = 2048 consecutive dwords (8 KiB) of a plane; its workgroup stages the plane's 256 table bytes
 *              once.
 *   HVQ_E_ARG for the whole call: null or misaligned tables; ntables outside 1 .. 65535; which == NULL with ntables other than 1 or n;
 *              a which[i] outside 0 .. ntables - 1; planes outside 1 .. 7; a null or misaligned dst[i]; n above 65535; a bad stream or
 *              ordinal; a src[i] with an ordinal other than -1 or that is no multiple of 16; a NULL context or dst.  n == 0 is HVQ_OK
 *              and does nothing.  Every argument is checked before anything is enqueued: a refused call leaves every destination
 *              untouched.  HVQ_E_NOGPU (after those checks) from a build without the map kernel.
 *   a_i and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_rank_pictures'. */
#define HVQ_MAP_TABLE_BYTES 768                     /* uint8 [3 planes Y, U, V][256] */
int     hvq_map_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                         const uint8_t *tables, int ntables, const int *which, int planes, void *const *dst, void *hip_stream);

/* TABLES FROM HISTOGRAM RECORDS, on the GPU: `hist` is `n` records exactly as hvq_picture_histograms writes them in HVQ_HIST_VALUES mode
 * (DEVICE memory, uint32 [3][256], 3072 bytes each, dense), `tables` `n` records of HVQ_MAP_TABLE_BYTES bytes in DEVICE memory; both
 * non-null multiples of 16.  One launch on the caller's stream, ordered behind whatever that stream holds, a member of the export chain;
 * every byte of `tables` is written, nothing else.  Record i goes through rules[which[i]] (which == NULL: rules[0] for all): luma for
 * plane Y, chroma for U and for V, each from its own histogram.  The entries are exact integers.  With h the plane's bins, N = sum h,
 * C(v) = h[0] + .. + h[v], and x_k (k from 1) the k-th smallest sample, i. e. the smallest v with C(v) >= k; `//` floors:
 *   HVQ_TBL_IDENTITY  lut[v] = v.
 *   HVQ_TBL_FLAT      lut[v] = a.
 *   N == 0            the identity, for each of the three kinds below.
 *   HVQ_TBL_EQUALIZE  C_min = the count of the smallest occurring value, D = N - C_min.  lut[v] = (2 * 255 * max(C(v) - C_min, 0) + D) //
 *                     (2 D); the identity when D == 0.  (hvqm4_amd.histograms.equalize_lut.)
 *   HVQ_TBL_STRETCH   a = clip_lo, b = clip_hi, per mille of the samples.  lo = x_k with k = max(1, ceil(a N / 1000)); hi = x_k with
 *                     k = max(1, ceil((1000 - b) N / 1000)) (the rank rule of histograms.percentile).  The identity when hi <= lo;
 *                     otherwise lut[v] = 0 for v <= lo, 255 for v >= hi, and (2 * 255 * (v - lo) + (hi - lo)) // (2 (hi - lo)) between.
 *   HVQ_TBL_OTSU      with n0 = C(t), n1 = N - n0, s0 = sum of v h[v] over v <= t, s1 the same over v > t and d = s0 n1 - s1 n0: t is the
 *                     t in 0 .. 254 with n0 > 0 and n1 > 0 that maximises d^2 / (n0 n1), the smallest such t on a tie, and 0 when there
 *                     is none (a single value).  Two scores compare exactly as d_a^2 (n0 n1)_b against d_b^2 (n0 n1)_a, in 192 bits.
 *                     lut[v] = 255 if v > t, else 0.  (histograms.otsu.)
 *   A record with N above 2^26 (no plane the library opens has more samples): the contents of its tables are unspecified; the call
 *   still writes only its bytes and computes in unsigned arithmetic that wraps.
 *   hvq_table_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL record or, in either plane: a kind outside the five; FLAT with a
 *   outside 0 .. 255; STRETCH with a or b outside 0 .. 499; a pad that is not 0; an a or b that is not 0 where the kind takes none (b
 *   under FLAT; both under IDENTITY, EQUALIZE and OTSU).
 *   HVQ_E_ARG for the whole call: what hvq_table_check refuses, in any entry, used or not; nrules outside 1 .. HVQ_TBL_MAX_RULES; a
 *   which[i] outside 0 .. nrules - 1; null or misaligned hist / tables; NULL rules; n above 65535; a NULL context.  n == 0 is HVQ_OK and
 *   does nothing.  Everything is checked before anything is enqueued.  HVQ_E_NOGPU (after those checks) from a build without the kernel. */
#define HVQ_TBL_IDENTITY 0
#define HVQ_TBL_FLAT     1   /* a = the value */
#define HVQ_TBL_EQUALIZE 2
#define HVQ_TBL_STRETCH  3   /* a = clip_lo, b = clip_hi, per mille of the samples, each 0 .. 499 */
#define HVQ_TBL_OTSU     4
#define HVQ_TBL_MAX_RULES 64
typedef struct HvqTablePlane { int32_t kind, a, b, pad; } HvqTablePlane;
typedef struct HvqTableRule  { HvqTablePlane luma, chroma; } HvqTableRule;   /* chroma serves U and V, each from its own histogram */
int     hvq_table_check(const HvqTableRule *r);
int     hvq_histogram_tables(HvqContext *ctx, int n, const uint32_t *hist, const HvqTableRule *rules, int nrules, const int *which,
                             uint8_t *tables, void *hip_stream);

/* CONNECTED COMPONENTS of resident pictures, where they lie: the foreground of ONE plane of each of `n` pictures, of any streams, sizes
 * and samplings, becomes a label map and a table of records, on the caller's HIP stream and without a host synchronisation.  It is the
 * step behind a mask (hvq_histogram_tables' OTSU, hvq_map_pictures, hvq_rank_pictures): how many blobs, where, how large.  This text is
 * the authority for the values.
 *   Foreground. Picture i goes through rules[which[i]] (which == NULL: rules[0] for all).  A sample a of plane rule.plane (0 Y, 1 U, 2 V;
 *              Nx x Ny samples at the plane's own resolution) is foreground when lo <= a <= hi.  lo = hi = 255 reads an Otsu mask.
 *   Components. The classes of the foreground under the 4-neighbourhood (left, right, above, below) or the 8-neighbourhood (the diagonals
 *              too) inside the plane: nothing wraps, nothing is replicated.  A component's FIRST SAMPLE is its sample of the smallest
 *              raster index y Nx + x.  Components are numbered 1 .. K in ascending order of their first samples (what a raster scan
 *              with a flood fill gives, and scipy.ndimage.label with the cross / the full 3 x 3 structure).
 *   labels[i]  a DEVICE pointer, a non-null multiple of 16: uint32 [Ny][Nx], dense, hvq_label_bytes bytes.  0 for background, k for a
 *              sample of component k.  Every element is written, whatever K and cap are; nothing outside is written.  While the work
 *              runs the map holds working values.
 *   comps[i]   a DEVICE pointer, a non-null multiple of 16: uint64 [cap + 1][8].  All values are below 2^63.
 *              Row 0 is {K, stored = min(K, cap), F = the number of foreground samples, status, 0, 0, 0, 0}.
 *              Row k, 1 <= k <= stored, is {area, x0, y0, x1, y1, first, sum_x, sum_y}: the number of samples, the bounding box
 *              (inclusive), the raster index of the first sample, and the exact sums of the samples' coordinates (the centroid is
 *              sum / area; a plane has at most 2^26 samples, nothing overflows).  Rows beyond `stored` are not touched.
 *              cap is 0 .. HVQ_LBL_MAX_CAP.
 *   status     0.  Every loop of the kernels has a bound that follows from the plane's size (a parent chain descends strictly, so it is
 *              no longer than the plane); a lane that reaches its bound stores HVQ_LBL_INCOMPLETE and leaves, and the values of that
 *              picture are then unspecified.  It does not happen unless something else writes the map while the work runs.
 *   Known answers.  An empty mask: K = 0, F = 0, labels all 0.  A full plane: K = 1, area Nx Ny, box (0, 0, Nx - 1, Ny - 1), first 0,
 *              sum_x = Ny Nx (Nx - 1) / 2, sum_y = Nx Ny (Ny - 1) / 2.  A 0 / 255 checkerboard under 4: K = the number of white
 *              samples, every area 1, label k at the k-th white sample in raster order; under 8: K = 1.  {255, 0; 0, 255}: K = 2
 *              under 4, K = 1 under 8.  A "U" whose arms start on row 0 is one component, label 1 on both arms.  The areas add up to F.
 *   hvq_label_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL rule, a plane outside 0 .. 2, a window that is not 0 <= lo <= hi <= 255,
 *              a connectivity other than 4 or 8.
 *   hvq_label_bytes (host only): 4 Nx Ny of that plane of such a picture; HVQ_E_GEOMETRY, or HVQ_E_ARG for the plane.
 *   The call.  Several launches behind one job table: a tile of HVQ_LB_TX x HVQ_LB_TY = 64 x 16 samples is labelled in LDS, the tiles'
 *              seams join by lock-free unions on the map, which is the parent array, the roots are numbered in raster order, and the
 *              records gather by 64-bit integer atomics: the values do not depend on the order of arrival.  No scratch memory.
 *   HVQ_E_ARG for the whole call: what hvq_label_check refuses, in any entry, used or not; nrules outside 1 .. HVQ_LBL_MAX_RULES; a
 *              which[i] outside 0 .. nrules - 1; cap outside 0 .. HVQ_LBL_MAX_CAP; a null or misaligned labels[i] or comps[i]; n above
 *              65535; a bad stream or ordinal; a src[i] with an ordinal other than -1 or that is no multiple of 16; a NULL context,
 *              rules, labels or comps.  n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is enqueued: a
 *              refused call leaves every output untouched.  HVQ_E_NOGPU (after those checks) from a build without the label kernels.
 *   a_i and `src` are hvq_picture_checksums'; lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain,
 *   slot safety and ending the batch in flight only when a requested picture belongs to it are hvq_rank_pictures'. */
#define HVQ_LBL_MAX_RULES 64
#define HVQ_LBL_MAX_CAP   (1 << 20)
#define HVQ_LBL_INCOMPLETE 1
typedef struct HvqLabelRule { int32_t plane, lo, hi, connectivity; } HvqLabelRule;
int     hvq_label_check(const HvqLabelRule *r);
int64_t hvq_label_bytes(int width, int height, int h_samp, int v_samp, int plane);   /* 4 * Nx * Ny of that plane */
int     hvq_label_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                           const HvqLabelRule *rules, int nrules, const int *which,
                           uint32_t *const *labels, uint64_t *const *comps, int cap, void *hip_stream);

/* LABELS BACK INTO PICTURES: output i is a uint8 picture in slot layout (Y | U | V) of the geometry of streams[i] -- the stream gives
 * the geometry only, no picture is looked up --, so the result composes with whatever takes `src`.  One launch of the map kernel's shape
 * on the caller's stream, a member of the export chain.
 *   Values.    With k the label of a Y sample and S = sel[which[i]] (which == NULL: sel[0] for all): the sample is SELECTED when
 *              1 <= k <= stored and area_min <= area <= area_max, w_min <= x1 - x0 + 1 <= w_max and h_min <= y1 - y0 + 1 <= h_max
 *              hold for record k.  The background and the labels without a record (k > stored) are not selected.  Y is 255 where
 *              selected, else 0; invert = 1 swaps the two, after that rule.  U and V are filled with 128.
 *              area_min alone is area opening: "remove the specks below N samples".
 *   Inputs.    labels[i] and comps[i] are hvq_label_pictures' outputs for the Y plane (a rule with plane 0) of a picture of that
 *              geometry, with the same cap.  They are read when the work runs: label -> select on one stream needs no host
 *              synchronisation.
 *   The call.  dst[i] is a non-null DEVICE pointer, a multiple of 16, of hvq_stream_pic_bytes bytes.  Exactly those bytes are written,
 *              each once; nothing outside them.
 *   HVQ_E_ARG for the whole call: nsel outside 1 .. HVQ_SEL_MAX; in any entry, used or not, a min above its max, an invert other than
 *              0 or 1, a pad that is not 0; a which[i] outside 0 .. nsel - 1; cap outside 0 .. HVQ_LBL_MAX_CAP; a null or misaligned
 *              labels[i], comps[i] or dst[i]; n above 65535; a bad stream; a NULL context, labels, comps, sel or dst.  n == 0 is HVQ_OK
 *              and does nothing.  Every argument is checked before anything is enqueued.  HVQ_E_NOGPU (after those checks) from a
 *              build without the kernel. */
#define HVQ_SEL_MAX 64
typedef struct HvqSelect { uint32_t area_min, area_max, w_min, w_max, h_min, h_max, invert, pad; } HvqSelect;
int     hvq_select_components(HvqContext *ctx, int n, const int *streams, const uint32_t *const *labels, const uint64_t *const *comps,
                              int cap, const HvqSelect *sel, int nsel, const int *which, void *const *dst, void *hip_stream);

/* CORNERS of resident pictures, where they lie: the trackable points of ONE plane of each of `n` pictures, of any streams, sizes and
 * samplings -- Harris' measure or the smaller eigenvalue of the structure tensor (Shi-Tomasi) --, as a mask picture, a row index and an
 * ordered list, on the caller's HIP stream and without a host synchronisation.  It is the step between a filter and motion: gradients
 * give edges, this gives the points a map can be fitted through.  This text is the authority for the values.  All values are exact
 * integers; nothing is rounded except the one floor square root.
 *   Samples.   Picture i goes through rules[which[i]] (which == NULL: rules[0] for all).  a*(y, x) = a[clamp(y)][clamp(x)] of plane
 *              rule.plane (0 Y, 1 U, 2 V; Nx x Ny samples at the plane's own resolution): borders are replicated, as in
 *              hvq_filter_pictures.
 *   Gradients. The 3 x 3 Sobel pair at any integer position, inside the plane or not:
 *              gx(y, x) = a*(y-1, x+1) + 2 a*(y, x+1) + a*(y+1, x+1) - a*(y-1, x-1) - 2 a*(y, x-1) - a*(y+1, x-1), gy its transpose
 *              (rows y+1 minus rows y-1).  |g| <= 4 * 255 = 1020.
 *   Sums.      Over the (2r + 1)^2 positions around (y, x), r = rule.radius in 1 .. HVQ_CRN_MAX_RADIUS, positions outside the plane
 *              included (their gradients read a*): A = sum gx^2, B = sum gx gy, C = sum gy^2, T = A + C.
 *              A, C <= 49 * 1020^2 = 50 979 600 < 2^26, |B| < 2^26 likewise, T < 2^27.
 *   Response.  R, int64.  HVQ_CRN_HARRIS: R = 256 (A C - B^2) - k T^2 with k in 1/256ths, 0 <= k <= 64 (k = 10 is the usual 0.04).
 *              A C >= B^2 (Cauchy-Schwarz), so 0 <= 256 (A C - B^2) < 2^8 * 2^52 = 2^60 and 0 <= k T^2 <= 2^6 * 2^54 = 2^60: |R| < 2^61.
 *              HVQ_CRN_MIN_EIGEN: R = T - isqrt((A - C)^2 + 4 B^2), isqrt the floor square root; the radicand is below 2^52 + 2^54 < 2^55
 *              and at most T^2, so 0 <= R < 2^27: R is twice the smaller eigenvalue, rounded up.  k must be 0 in this mode.
 *   Corners.   A sample p = (x, y) is a corner when margin <= x < Nx - margin and margin <= y < Ny - margin (0 <= margin <= 255),
 *              R(p) >= threshold (threshold >= 1), and no sample q != p OF THE PLANE with |qx - px| <= nms and |qy - py| <= nms beats
 *              it.  q beats p when R(q) > R(p), or R(q) == R(p) and q's raster index y Nx + x is the smaller.  Samples in the margin
 *              still suppress.  nms = 0 keeps every sample over the threshold.  The order is total: the result does not depend on the
 *              order of evaluation.
 *   mask[i]    a DEVICE pointer, a non-null multiple of 16: a uint8 picture in slot layout of the geometry of streams[i],
 *              hvq_stream_pic_bytes bytes, every byte written once.  The analysed plane holds 255 at corners and 0 elsewhere; of the
 *              planes that were not analysed Y is filled with 0, U and V with 128.  It goes wherever `src` goes.
 *   rows[i]    a DEVICE pointer, a non-null multiple of 16: uint32 [Ny + 1], hvq_corner_rows_bytes bytes.  rows[y] is the number of
 *              corners in the rows above y, rows[Ny] = K: a row index into the list.  While the work runs it holds working values.
 *   points[i]  a DEVICE pointer, a non-null multiple of 16: int64 [cap + 1][4], cap in 0 .. HVQ_CRN_MAX_CAP.  Row 0 is {K, stored =
 *              min(K, cap), status = 0, 0}.  Row j, 1 <= j <= stored, is {x, y, R, y Nx + x}, in ascending raster order.  Rows beyond
 *              `stored` are not touched.
 *   response   NULL, or an array of n entries, each NULL or a DEVICE pointer, a multiple of 16: int64 [Ny][Nx],
 *              hvq_corner_response_bytes bytes, every R of the plane.
 *   Known answers (both modes, r = 1, 2, 3).  A flat plane: K = 0 under every rule.  One straight vertical 0 | 255 edge: R <= 0 (Harris)
 *              or R = 0 (min-eigenvalue) everywhere, K = 0.  A 0 / 255 checkerboard of single samples: R = 0 at every sample further
 *              than r + 1 from the border (both Sobel columns have the same parity there); with nms = 1 and threshold = 1 its corners
 *              are exactly the four corners of the plane.  Stripes of period 4 (0, 0, 255, 255 along x): every |gx| = 1020, gy = 0;
 *              under Harris with k = 64 and r = 3 the most negative R is -64 (49 * 1020^2)^2 = -166 330 855 434 240 000, which needs 58
 *              bits; under min-eigenvalue R = 0 everywhere.  A 32 x 24 plane that is 255 for y >= 10, x >= 13 and 0 elsewhere, under
 *              Harris with r = 1, k = 10, nms = 3, threshold = 1: exactly one corner, (x, y) = (13, 10) with R = 2 192 466 340 080 000;
 *              with r = 2 it is (14, 11), with r = 3 (15, 12).
 *   hvq_corner_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL rule, a plane outside 0 .. 2, an unknown mode, a radius outside
 *              1 .. HVQ_CRN_MAX_RADIUS, k outside 0 .. 64 or k != 0 under HVQ_CRN_MIN_EIGEN, nms outside 0 .. HVQ_CRN_MAX_NMS, a margin
 *              outside 0 .. 255, threshold < 1, a pad that is not 0.
 *   hvq_corner_rows_bytes, hvq_corner_response_bytes (host only): 4 (Ny + 1) and 8 Nx Ny of that plane of such a picture;
 *              HVQ_E_GEOMETRY, or HVQ_E_ARG for the plane.
 *   The call.  Four launches behind one job table, and no memory besides the outputs: a workgroup stages a 64 x 16 tile with a halo of
 *              nms + r + 1, takes the gradients once per position, slides the three sums along the rows and down the columns, leaves
 *              the responses of the tile and its nms halo in LDS and suppresses from there; a wave a row counts the mask's corners;
 *              one workgroup a picture scans the counts into rows and writes row 0 of points; a wave a row places its corners.
 *   HVQ_E_ARG for the whole call: what hvq_corner_check refuses, in any entry, used or not; nrules outside 1 .. HVQ_CRN_MAX_RULES; a
 *              which[i] outside 0 .. nrules - 1; cap outside 0 .. HVQ_CRN_MAX_CAP; a null or misaligned mask[i], points[i] or rows[i]; a
 *              misaligned response[i]; n above 65535; a bad stream or ordinal; a src[i] with an ordinal other than -1 or that is no
 *              multiple of 16; a NULL context, rules, mask, points or rows.  n == 0 is HVQ_OK and does nothing.  Every argument is
 *              checked before anything is enqueued: a refused call leaves every output untouched.  HVQ_E_NOGPU (after those checks)
 *              from a build without the corner kernels.
 *   a_i and `src`, lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain, slot safety and ending the
 *   batch in flight only when a requested picture belongs to it are hvq_label_pictures'. */
#define HVQ_CRN_MAX_RULES   64
#define HVQ_CRN_MAX_CAP     (1 << 20)
#define HVQ_CRN_MAX_RADIUS  3      /* structure window (2r+1)^2, r in 1..3 */
#define HVQ_CRN_MAX_NMS     7
#define HVQ_CRN_HARRIS      0
#define HVQ_CRN_MIN_EIGEN   1
typedef struct HvqCornerRule { int32_t plane, mode, radius, k, nms, margin, pad[2]; int64_t threshold; } HvqCornerRule;  /* 40 bytes */
int     hvq_corner_check(const HvqCornerRule *r);
int64_t hvq_corner_rows_bytes(int width, int height, int h_samp, int v_samp, int plane);      /* 4 (Ny + 1) */
int64_t hvq_corner_response_bytes(int width, int height, int h_samp, int v_samp, int plane);  /* 8 Nx Ny */
int     hvq_corner_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                            const HvqCornerRule *rules, int nrules, const int *which,
                            uint8_t *const *mask, int64_t *const *points, uint32_t *const *rows, int64_t *const *response,
                            int cap, void *hip_stream);

/* EXACT DISTANCE TRANSFORMS of resident pictures, where they lie: for ONE plane of each of `n` pictures, of any streams, sizes and
 * samplings, how far every foreground sample is from the background, on the caller's HIP stream and without a host synchronisation.
 * It is the step behind a mask that labelling is not: erosion and dilation by a disc of any radius, the thickness of an object, seeds
 * for splitting touching blobs, a signed field, buffer zones.  This text is the authority for the values.
 *   Foreground. Picture i goes through rules[which[i]] (which == NULL: rules[0] for all).  A sample a of plane rule.plane (0 Y, 1 U, 2 V;
 *              Nx x Ny samples at the plane's own resolution) is foreground when lo <= a <= hi, as in HvqLabelRule; everything else is
 *              background.  The distance of the background to the foreground is the same call with the complementary window; a signed
 *              field is two calls.
 *   dist[i]    a DEVICE pointer, a non-null multiple of 16: uint32 [Ny][Nx], dense, hvq_distance_bytes bytes.  0 at a background
 *              sample.  At a foreground sample (x, y) the minimum over all background samples (bx, by) of the plane of
 *              (bx - x)^2 + (by - y)^2 under HVQ_DST_EUCLID2, |bx - x| + |by - y| under HVQ_DST_CITY, max(|bx - x|, |by - y|) under
 *              HVQ_DST_CHESS.  With border = 1 the samples just outside the plane count as background too, which adds the candidate
 *              e = min(x + 1, Nx - x, y + 1, Ny - y): e^2 under EUCLID2, e under the other two; with border = 0 nothing outside the
 *              plane exists.  A foreground sample with no candidate at all (a plane without background, border = 0) holds
 *              HVQ_DST_NONE.  Nothing is rounded; the largest plane is 8192 x 8192, so every other value is below 2^27.  Every
 *              element is written once the call has run, nothing outside the map is written; while the work runs the map holds
 *              working values.
 *   Known answers.  An all-background plane: all 0.  A full 8 x 5 plane with border = 0: all HVQ_DST_NONE; with border = 1 under
 *              EUCLID2 the rows 1 1 1 1 1 1 1 1 / 1 4 4 4 4 4 4 1 / 1 4 9 9 9 9 4 1 / 1 4 4 4 4 4 4 1 / 1 1 1 1 1 1 1 1.  An 8 x 6
 *              plane whose only background sample is (0, 0) has 7^2 + 5^2 = 74 at (7, 5), 12 under CITY and 7 under CHESS.
 *   hvq_distance_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL rule, a plane outside 0 .. 2, a window that is not
 *              0 <= lo <= hi <= 255, a metric outside 0 .. 2, a border outside 0 .. 1, a pad that is not 0.
 *   hvq_distance_bytes (host only): 4 Nx Ny of that plane of such a picture; HVQ_E_GEOMETRY, or HVQ_E_ARG for the plane.
 *   The call.  Two launches behind one job table, and no memory besides the map: a lane walks four columns down and up and leaves the
 *              vertical distances in the map; a workgroup stages whole rows of them (HVQ_DT_SPAN = 8192 samples, uint16) in LDS and
 *              overwrites the rows in place with the minimum over the row, searching outwards from each sample until nothing further
 *              out can win.  Integers only: the values do not depend on any order.
 *   HVQ_E_ARG for the whole call: what hvq_distance_check refuses, in any entry, used or not; nrules outside 1 .. HVQ_DST_MAX_RULES; a
 *              which[i] outside 0 .. nrules - 1; a null or misaligned dist[i]; n above 65535; a bad stream or ordinal; a src[i] with
 *              an ordinal other than -1 or that is no multiple of 16; a NULL context, rules or dist.  n == 0 is HVQ_OK and does
 *              nothing.  Every argument is checked before anything is enqueued: a refused call leaves every output untouched.
 *              HVQ_E_NOGPU (after those checks) from a build without the distance kernels.
 *   a_i and `src`, lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain and slot safety are
 *   hvq_label_pictures'. */
#define HVQ_DST_EUCLID2 0
#define HVQ_DST_CITY    1
#define HVQ_DST_CHESS   2
#define HVQ_DST_NONE    0xFFFFFFFFu
#define HVQ_DST_MAX_RULES 64
typedef struct HvqDistanceRule { int32_t plane, lo, hi, metric, border, pad[3]; } HvqDistanceRule;
int     hvq_distance_check(const HvqDistanceRule *r);
int64_t hvq_distance_bytes(int width, int height, int h_samp, int v_samp, int plane);   /* 4 * Nx * Ny of that plane */
int     hvq_distance_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                              const HvqDistanceRule *rules, int nrules, const int *which,
                              uint32_t *const *dist, void *hip_stream);

/* DISTANCES BACK INTO PICTURES: output i is a uint8 picture in slot layout (Y | U | V) of the geometry of streams[i] -- the stream gives
 * the geometry only, no picture is looked up --, so the result composes with whatever takes `src`.  One launch of the map kernel's shape
 * on the caller's stream, a member of the export chain.
 *   Values.    With d the distance of a Y sample and S = sel[which[i]] (which == NULL: sel[0] for all).  HVQ_DSM_RANGE: Y is 255 where
 *              lo <= d <= hi, else 0; invert = 1 swaps the two, after that rule.  HVQ_DST_NONE is an ordinary value here: hi =
 *              0xFFFFFFFF includes it.  HVQ_DSM_ROOT: Y is min(255, isqrt(d)), isqrt the exact integer floor square root, so
 *              HVQ_DST_NONE gives 255; lo, hi and invert must be 0.  It is the viewable field under EUCLID2.  U and V are filled
 *              with 128.
 *              Erosion by a disc of radius r is hvq_distance_pictures (EUCLID2) -> RANGE [r^2 + 1, HVQ_DST_NONE]; dilation by a disc
 *              is the same on the complementary window, inverted.
 *   Inputs.    dist[i] is a map of the Y plane (a rule with plane 0) of a picture of that geometry, read when the work runs: distance
 *              -> mask on one stream needs no host synchronisation.
 *   The call.  dst[i] is a non-null DEVICE pointer, a multiple of 16, of hvq_stream_pic_bytes bytes.  Exactly those bytes are written,
 *              each once; nothing outside them.
 *   HVQ_E_ARG for the whole call: nsel outside 1 .. HVQ_DSM_MAX; in any entry, used or not, lo above hi, a mode outside 0 .. 1, an
 *              invert other than 0 or 1, a pad that is not 0, under ROOT a lo, hi or invert that is not 0; a which[i] outside
 *              0 .. nsel - 1; a null or misaligned dist[i] or dst[i]; n above 65535; a bad stream; a NULL context, dist, sel or dst.
 *              n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is enqueued.  HVQ_E_NOGPU (after those
 *              checks) from a build without the kernel. */
#define HVQ_DSM_RANGE 0
#define HVQ_DSM_ROOT  1
#define HVQ_DSM_MAX 64
typedef struct HvqDistanceMask { uint32_t mode, lo, hi, invert, pad[4]; } HvqDistanceMask;
int     hvq_distance_mask_check(const HvqDistanceMask *m);
int     hvq_distance_mask(HvqContext *ctx, int n, const int *streams, const uint32_t *const *dist,
                          const HvqDistanceMask *sel, int nsel, const int *which, void *const *dst, void *hip_stream);

/* SUMMED-AREA TABLES of resident pictures, where they lie: for ONE plane of each of `n` pictures, of any streams, sizes and samplings,
 * the inclusive table of sums and, where asked, of squares, on the caller's HIP stream and without a host synchronisation.  A table makes
 * the sum of a window of ANY size cost four reads: local means and deviations over windows far wider than the filter and rank calls
 * reach, thresholds relative to them (a page, a vignette, a night scene with one lamp, where one threshold a plane fails), the mean
 * brightness of every box that hvq_label_pictures found, Haar-like features.  This text is the authority for the values.
 *   Tables.    Picture i contributes plane which_plane[i] (0 Y, 1 U, 2 V; Nx x Ny samples a at the plane's own resolution;
 *              which_plane == NULL: Y of all).  sums[i] is a DEVICE pointer, a non-null multiple of 16: uint32 [Ny][Nx], dense,
 *                  S(x, y) = sum of a(x', y') over x' <= x, y' <= y,   modulo 2^32.
 *              A plane holds up to 2^26 samples, so S wraps, by design: the sum of a rectangle of at most 2^24 samples comes out exact
 *              from the wrapped corners in uint32 arithmetic, because 255 * 2^24 < 2^32.  `squares` may be NULL; where squares[i] is
 *              non-null it is a multiple of 16, uint64 [Ny][Nx], Q(x, y) = the same sum of a^2, which never wraps (2^26 * 255^2 < 2^64).
 *              The tables are INCLUSIVE, not the (Ny + 1) x (Nx + 1) tables of other libraries: rows stay multiples of 16 bytes.  A
 *              corner at x = -1 or y = -1 reads as 0.  Every element is written once the call has run, nothing outside the tables;
 *              while the work runs they hold working values.
 *   hvq_integral_bytes (host only): 4 Nx Ny (order 1) or 8 Nx Ny (order 2) of that plane of such a picture; HVQ_E_GEOMETRY, or HVQ_E_ARG
 *              for the plane or the order.
 *   The call.  Two launches behind one job table, and no memory besides the tables: a wave scans a row a dword of the plane a lane a
 *              step (HVQ_IG_CHUNK = 256 samples a step: the prefix of the lanes' totals by shuffles, a carry from step to step); then a
 *              lane walks four columns downwards in place.  Integers only: the values do not depend on any order.
 *   HVQ_E_ARG for the whole call: a which_plane[i] outside 0 .. 2; a null or misaligned sums[i]; a misaligned squares[i]; n above
 *              65535; a bad stream or ordinal; a src[i] with an ordinal other than -1 or that is no multiple of 16; a NULL context or
 *              sums.  n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is enqueued: a refused call leaves
 *              every output untouched.  HVQ_E_NOGPU (after those checks) from a build without the integral kernels.
 *   a_i and `src`, lookup, the HVQ_E_STATE cases, ordering on `hip_stream`, membership of the export chain and slot safety are
 *   hvq_distance_pictures'. */
int64_t hvq_integral_bytes(int width, int height, int h_samp, int v_samp, int plane, int order);   /* 4 or 8 * Nx * Ny of that plane */
int     hvq_integral_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                              const int *which_plane, uint32_t *const *sums, uint64_t *const *squares, void *hip_stream);

/* TABLES BACK INTO PICTURES: output i is a uint8 picture in slot layout (Y | U | V) of the geometry of streams[i]; Y holds the result, U
 * and V are filled with 128, exactly as hvq_distance_mask does, so the result goes wherever `src` goes.  One launch on the caller's
 * stream, a member of the export chain.
 *   Inputs.    Picture i goes through rules[which[i]] (which == NULL: rules[0] for all).  sums[i] (and squares[i]) are the tables of
 *              plane rule.plane of picture i as hvq_integral_pictures left them, read when the work runs: integral -> window on one
 *              stream needs no host synchronisation.  That plane must have the size of Y: plane 0, or any plane of a 4:4:4 picture.
 *              The picture itself (a_i, `src`, lookup as in hvq_integral_pictures) is read by HVQ_WIN_THRESHOLD only.
 *   Window.    The window of sample (x, y) is [x - rx, x + rx] x [y - ry, y + ry], CUT TO THE PLANE: nothing is replicated.  Let n be
 *              the number of samples left in the window, S their sum and Q their sum of squares, a the sample itself.
 *   HVQ_WIN_MEAN       (2 S + n) / (2 n) rounded down: the mean rounded half up.  It is the only rounding.
 *   HVQ_WIN_DEVIATION  the largest d with (d n)^2 <= n Q - S^2: the floor of the population standard deviation, always in 0 .. 127.
 *   HVQ_WIN_THRESHOLD  255 where 256 n a > 256 S + k d n - 256 c n, else 0, with d as in HVQ_WIN_DEVIATION; invert = 1 swaps the two.
 *              It reads as a > mean + (k / 256) d - c: k = 0 is the "mean - C" rule and needs no squares, k != 0 is Niblack's rule on
 *              the integer deviation.  k in -1024 .. 1024, c in -255 .. 255: everything fits int64.  The other two modes ignore k, c
 *              and invert.
 *   Known answers.  A plane of constant v: MEAN v, DEVIATION 0, THRESHOLD with k = 0 gives 0 for c <= 0 and 255 for c > 0.  A 0 / 255
 *              checkerboard wherever the cut window has an even number of samples: DEVIATION 127.  rx >= Nx and ry >= Ny: every sample
 *              sees the whole plane.  An 8192 x 2064 plane of 255: S(Nx - 1, Ny - 1) = 4 311 613 440 mod 2^32 = 16 646 144, and the
 *              rectangle x 100 .. 8191, y 10 .. 2057 (16 572 416 samples) still gives exactly 255 * 16 572 416.
 *   hvq_window_check (host only): HVQ_OK, or HVQ_E_ARG for a NULL rule, a plane outside 0 .. 2, a mode outside 0 .. 2, rx or ry outside
 *              0 .. 8191, k outside -1024 .. 1024, c outside -255 .. 255, an invert other than 0 or 1, a pad that is not 0.
 *   The call.  dst[i] is a non-null DEVICE pointer, a multiple of 16, of hvq_stream_pic_bytes bytes.  Exactly those bytes are written,
 *              each once; nothing outside them.  A workgroup takes 64 x 16 samples of Y, a lane four adjacent ones.
 *   HVQ_E_ARG for the whole call: what hvq_window_check refuses, in any entry, used or not; nrules outside 1 .. HVQ_WIN_MAX_RULES; a
 *              which[i] outside 0 .. nrules - 1; min(2 rx + 1, Nx) * min(2 ry + 1, Ny) above 2^24 for any picture; a rule that needs Q
 *              (DEVIATION, THRESHOLD with k != 0) where `squares` or squares[i] is NULL; a rule whose plane has not the size of Y; a
 *              null or misaligned sums[i] or dst[i], a misaligned squares[i]; n above 65535; a bad stream or ordinal, a bad src[i]; a
 *              NULL context, sums, rules or dst.  n == 0 is HVQ_OK and does nothing.  Every argument is checked before anything is
 *              enqueued.  HVQ_E_NOGPU (after those checks) from a build without the kernel. */
#define HVQ_WIN_MEAN      0
#define HVQ_WIN_DEVIATION 1
#define HVQ_WIN_THRESHOLD 2
#define HVQ_WIN_MAX_RULES 64
#define HVQ_WIN_MAX_RADIUS 8191
typedef struct HvqWindowRule { int32_t plane, mode, rx, ry, k, c, invert, pad; } HvqWindowRule;
int     hvq_window_check(const HvqWindowRule *r);
int     hvq_window_pictures(HvqContext *ctx, int n, const int *streams, const int *ordinals, const void *const *src,
                            const uint32_t *const *sums, const uint64_t *const *squares, const HvqWindowRule *rules, int nrules,
                            const int *which, void *const *dst, void *hip_stream);

/* SUMS OF RECTANGLES from the tables of `n` pictures, the rectangles IN DEVICE MEMORY: the boxes of hvq_label_pictures' records become
 * rectangles by an expression on the device, with no synchronisation.  One launch, a lane a rectangle and eight loads, a member of the
 * export chain.
 *   rects      a DEVICE pointer, a multiple of 4: int32 [nrects][5] = (i, x0, y0, x1, y1), corners inclusive, i the picture.
 *   sums, squares   host arrays of n DEVICE pointers as in hvq_integral_pictures; squares or squares[i] NULL: Q comes out 0.
 *   dims       a DEVICE pointer, a multiple of 4: uint32 [n][2] = (Nx, Ny) of the tables.
 *   out        a DEVICE pointer, a multiple of 8: uint64 [nrects][3] = (count, S, Q).  A rectangle that leaves its plane, is empty
 *              (x1 < x0 or y1 < y0), has more than 2^24 samples or names an i outside 0 .. n - 1 gives (0, 0, 0): the call cannot
 *              check device data on the host.  Every element is written.
 *   HVQ_E_ARG: n outside 1 .. 65535 or nrects outside 0 .. 2^24 (nrects == 0 is HVQ_OK and does nothing); a null or misaligned
 *              rects, dims, out or sums[i], a misaligned squares[i]; a NULL context or sums.  HVQ_E_NOGPU after those checks. */
#define HVQ_RECT_MAX (1 << 24)
int     hvq_rect_sums(HvqContext *ctx, int n, int nrects, const int32_t *rects, const uint32_t *const *sums, const uint64_t *const *squares,
                      const uint32_t *dims, uint64_t *out, void *hip_stream);

/* Measurement helper: `reps` copies of `bytes` from pinned host memory to the device on the context's copy stream, HIP-event timed:
 * the PCIe rate the upload of a batch's bitstreams can reach on this box (GB/s, 1e9). */
int  hvq_h2d_probe(HvqContext *ctx, size_t bytes, int reps, double *gb_per_s);

int  hvq_get_stats(HvqContext *ctx, HvqStats *out);
/* self-test of the kernels' replacement for the reference's division tables (h4m:265-273): out[0..15] = 256 / d, out[16..271] = 4096 / d
 * as the device computes them (0 for d = 0) */
int  hvq_debug_table_divisions(HvqContext *ctx, uint32_t *out);
const char *hvq_last_error_string(void);

/* .h4m container demux in memory (header checks of load_header h4m:2175-2247, block/record walk of h4m:2427-2537).
 * Host only.  Typical use:
 *     HvqH4mInfo info; hvq_h4m_header(file, n, &info);
 *     int sid = hvq_stream_open(ctx, info.width, info.height, info.h_samp, info.v_samp, info.is_1_5, 6);
 *     HvqH4mIter it; hvq_h4m_begin(&it);
 *     while (hvq_h4m_next(file, n, &it, &type, &disp, &pic, &len) == 1) hvq_stream_submit(ctx, sid, type, pic, len);
 *     hvq_flush(ctx);                                                                                         */
typedef struct HvqH4mInfo {
    uint32_t header_size, body_size, blocks, video_frames, audio_frames, usec_per_frame, max_frame_size;
    uint32_t pic_bytes;            /* w*h*(hs*vs+2)/(hs*vs), h4m:2343-2345 */
    uint16_t width, height;
    uint8_t  h_samp, v_samp, video_mode, is_1_5;
} HvqH4mInfo;
typedef struct HvqH4mIter {
    size_t   pos, block_end;
    uint32_t block, v_left, a_left, video_seen, gop_start, in_block;
} HvqH4mIter;
int  hvq_h4m_header(const uint8_t *data, size_t n, HvqH4mInfo *out);
void hvq_h4m_begin(HvqH4mIter *it);
/* 1: produced a video picture (`pic` = data after the disp_id word, `disp_id` = gop_start + record disp_id);
 * 0: clean end of file; < 0: HVQ_E_CONTAINER */
int  hvq_h4m_next(const uint8_t *data, size_t n, HvqH4mIter *it, int *frame_type, uint32_t *disp_id,
                  const uint8_t **pic, size_t *len);

/* Host-only pieces, usable without a GPU (parse is pixel-independent). */
typedef struct HvqParser HvqParser;
HvqParser *hvq_parser_create(int width, int height, int h_samp, int v_samp, int is_1_5);
void hvq_parser_destroy(HvqParser *p);
size_t hvq_parser_blob_bound(const HvqParser *p);
uint32_t hvq_parser_pic_bytes(const HvqParser *p);
int  hvq_parse_picture(HvqParser *p, int frame_type, const uint8_t *pic, size_t len,
                       uint8_t *blob, size_t cap, size_t *blob_len);
/* Length of a picture from its own section table (what the SDK entry points, whose signatures carry no length, parse with).
 * `limit` = readable bytes at `pic` (0 = unknown: the table's words are trusted like the reference trusts them). */
int  hvq_picture_length(const uint8_t *pic, int frame_type, uint32_t limit, size_t *len);

#ifdef __cplusplus
}
#endif
#endif
