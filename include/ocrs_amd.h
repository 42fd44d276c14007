/*
 * ocrs_amd.h — C ABI of the MI355X-native OCR engine (libocrs_amd.so).
 *
 * This is the drop-in boundary for the hot path of robertknight/ocrs
 * (prepare_input -> detect_words -> find_text_lines -> recognize_text).  Every
 * entry point names the reference interface it replaces (paths relative to
 * the reference tree).  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns an ocrs_status; on failure ocrs_last_error()
 *     (thread-local) holds the message the reference would have put into its
 *     anyhow::Error / ModelRunError (ocrs/src/errors.rs:6-25).  Nothing aborts.
 *   - all handles are safe to use from several host threads at once (the
 *     reference calls Model::run concurrently from a rayon pool,
 *     ocrs/src/recognition.rs:465-485; models are `Send + Sync`,
 *     detection.rs:67, recognition.rs:316).
 *   - buffers returned through `T**` are allocated by the library and released
 *     with ocrs_buffer_free().
 *   - a RotatedRect crosses the boundary as 6 floats:
 *     center.x, center.y, up.x, up.y, width, height
 *     (rten_imageproc::RotatedRect::new(center, up_axis, width, height),
 *     ctor order shown at recognition.rs:582).
 */
#ifndef OCRS_AMD_H
#define OCRS_AMD_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define OCRS_API __attribute__((visibility("default")))
#else
#define OCRS_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ocrs_status {
    OCRS_OK = 0,
    OCRS_ERR_INVALID_ARGUMENT = 1,
    OCRS_ERR_MODEL_NOT_LOADED = 2, /* lib.rs:197,211,254,274 */
    OCRS_ERR_MODEL_DIMS = 3,       /* detection.rs:141-144 "failed to get model dims" */
    OCRS_ERR_RUN_FAILED = 4,       /* ModelRunError::RunFailed, errors.rs:8 */
    OCRS_ERR_WRONG_OUTPUT = 5,     /* ModelRunError::WrongOutput, errors.rs:11 */
    OCRS_ERR_IMAGE_SOURCE = 6,     /* ImageSourceError, preprocess.rs:38-46 */
    OCRS_ERR_DEVICE = 7,           /* HIP runtime failure / no GPU */
    OCRS_ERR_IO = 8,
    OCRS_ERR_CAPACITY = 9
} ocrs_status;

/* Message for the last failure on the calling thread ("" if none). */
OCRS_API const char* ocrs_last_error(void);

/* Layout version of the parameter structs below (ocrs_engine_params, ocrs_group_params) and of the argument lists: a binding
 * compares ocrs_abi_version() with the OCRS_ABI_VERSION it was built against when it loads the library and refuses a
 * mismatch, instead of passing a struct the library reads past the end of.  Bumped whenever a struct grows or an argument
 * list changes (6 = round 6; rounds 1-5 had no version: their structs were shorter).  Names of options removed since are
 * still accepted by ocrs_set_option and ignored. */
#define OCRS_ABI_VERSION 6u
OCRS_API uint32_t ocrs_abi_version(void);

/* Release any buffer handed out through a `T**` out-parameter. */
OCRS_API void ocrs_buffer_free(void* p);

/* Devices.  Every handle (model, engine, page) belongs to ONE HIP device, and every entry point binds the calling
 * host thread to its handle's device for the duration of the call: one process may hold engines on several GPUs
 * (and use them from any thread), or one process per GPU may each use its own.  The reference engine is immutable
 * `&self` (ocrs/src/lib.rs:183-256), which is what makes both shapes natural.
 *   ocrs_device_count  HIP devices visible
 *   ocrs_set_device    the DEFAULT device: where handles created without an explicit device live (the
 *                      one-process-per-GPU deployment calls it once, with LOCAL_RANK; initially 0)
 *   ocrs_get_device    the current default */
OCRS_API ocrs_status ocrs_device_count(int* n);
OCRS_API ocrs_status ocrs_set_device(int device);
OCRS_API ocrs_status ocrs_get_device(int* device);

/* rten::ctc::CtcDecoder::decode_beam (as called at ocrs/src/recognition.rs:512-514) on a host matrix of
 * log-probabilities [T][C] (blank = class 0): the steps (label, position) of the best prefix.  `impl`: 0 = the
 * host implementation the engine uses, 1 = the same function written as the algorithm is usually stated (slow;
 * the test oracle of 0), 2 = the HIP kernel the engine uses for DecodeMethod::BeamSearch (uploads the matrix).
 * Outputs are malloc'ed (ocrs_buffer_free). */
OCRS_API ocrs_status ocrs_ctc_beam_search(const float* logp, int t, int c, uint32_t width, int impl, uint32_t** labels,
                                          uint32_t** positions, size_t* n);
/* The same with confidence: *score = the best beam's float64 lse(pb, pnb) (0 if t = 0), *step_logp[i] = logp[pos_i][label_i]
 * (n entries, malloc'ed). */
OCRS_API ocrs_status ocrs_ctc_beam_search_scored(const float* logp, int t, int c, uint32_t width, int impl, uint32_t** labels,
                                                 uint32_t** positions, size_t* n, double* score, float** step_logp);

/* Test hook: the decode stage of a packed recognition batch (everything after the head GEMM) on chosen head outputs.
 * `logits`: the n lines' head outputs [lengths[i]][c], line after line, lines in the caller's order (a length may be 0);
 * `excluded`: [c] flags by label, or NULL.  method: 0 greedy, 1 greedy scored, 2 beam search (the HIP kernel, `width`
 * beams), 3 beam search scored.  The lines are sorted and packed as a request's are (longest first, row t of line slot m at
 * packed row off[t] + m), run through the LogSoftmax + arg-max kernel and then through the same function the engine's
 * requests end in.  Outputs, per line in the caller's order: the steps of line i are labels / positions
 * [step_offsets[i], step_offsets[i + 1]) (step_offsets: n + 1 entries, the caller's; labels / positions malloc'ed);
 * scored methods (step_logp and scores required, else ignored): *step_logp indexed like the steps (malloc'ed), scores[i]
 * the line score (0 for a line of length 0); logp (optional): *logp = the lines' unmasked log-probs [lengths[i]][c], line
 * after line (malloc'ed).  OCRS_ERR_CAPACITY: beam search with a (c, width) the kernel does not support. */
OCRS_API ocrs_status ocrs_ctc_decode_packed(const float* logits, const int32_t* lengths, size_t n, int c, const uint8_t* excluded,
                                            int method, uint32_t width, uint32_t** labels, uint32_t** positions,
                                            size_t* step_offsets, float** step_logp, double* scores, float** logp);

/* Test hook: the component stage of detection (find_connected_component_rects, detection.rs:41-62) on chosen masks.
 * `masks`: n pages [h][w] of 0 / 1 bytes on the host.  They are uploaded and go through the component labelling and the
 * contour / rectangle kernel as a detection request's masks do (RDP eps 2, the process's `ccl_quad` option), with the
 * caller's `expand`, `min_area` and scratch sizes: `max_comp` component slots and `arena` border points per page.  Outputs
 * (the caller's arrays), per page: n_roots[i] the number of components found (also when it exceeds max_comp), overflow[i]
 * non-zero when the page did not fit max_comp or arena, rects [n][max_comp][6] (cx, cy, upx, upy, w, h) and valid
 * [n][max_comp].  Slot c < min(n_roots[i], max_comp) is the page's c-th component in raster order of its first pixel;
 * valid 1: the rect is written and w * h >= min_area; valid 0: no rect or too small (the floats are then unspecified).  A
 * slot the kernel did not write at all holds valid 0xEE.  On an overflowed page which slots were filled is unspecified.
 * OCRS_ERR_INVALID_ARGUMENT: h or w outside 1 .. 65535, max_comp < 1, arena < 1 or >= 2^31, or a batch beyond the hook's
 * bounds (64 pages, 2^26 pixels, 2^26 arena points, 2^24 slots in all). */
OCRS_API ocrs_status ocrs_mask_component_rects(const uint8_t* masks, size_t n, int h, int w, float expand, float min_area,
                                               int max_comp, int64_t arena, int32_t* n_roots, int32_t* overflow, float* rects,
                                               uint8_t* valid);

/* Test hook (host only, no GPU work): how the persistent GRU kernel would deal the 16-line row tiles of a request
 * to its waves.  lengths_desc = sequence lengths of the lines, descending (tile k = lines 16k .. 16k+15).
 * *n_clusters = clusters per direction, *waves = 4 = wave slots per cluster; tiles[4s .. 4s+3] for slot
 * s = cluster * 4 + wave.  Tile indices longest first, -1 = none.  OCRS_ERR_CAPACITY if the shape has no persistent plan. */
OCRS_API ocrs_status ocrs_gru_tile_plan(const int32_t* lengths_desc, size_t n_lines, int hidden, int32_t* n_clusters, int32_t* waves,
                                        int16_t* tiles);

/* Test hook (host only, no GPU work) for the request coalescer behind the one-page entry points (ocrs_engine_params.coalesce):
 * n_threads callers submit requests_per_thread requests each (of two incompatible kinds, weights 1..2 pages); request
 * ids divisible by fail_every (> 0) fail.  out = {batches run, requests carried, errors delivered to their callers,
 * requests that were run twice / not at all / got a wrong result or shared a batch with the other kind, largest batch
 * in pages}. */
OCRS_API ocrs_status ocrs_coalescer_selftest(int n_threads, int requests_per_thread, int max_active, int max_pages,
                                             long window_us, int fail_every, uint64_t out[5]);

/* Test hook (host only, no GPU work) for the stream plan of a device (option "stream_budget"): a plan of `budget` streams is
 * driven through n_ops operations, ops = n_ops pairs {op, arg}, one result each in out:
 *   0 a call starts, avoiding light lane arg (-1: none) -> its light lane, -1 = a stream of its own (budget 0)
 *   1 a call on lane arg ends                           -> calls still in flight
 *   2 the budget becomes arg                            -> 1 taken up, 0 refused (a call is in flight, or not 0 / 3 .. 16)
 *   3 calls on light lane arg, 4 the budget, 5 the number of light lanes. */
OCRS_API ocrs_status ocrs_stream_plan_selftest(int budget, const int32_t* ops, size_t n_ops, int32_t* out);

/* Test hook (host only, no GPU work) for the two host decisions behind "conv_rows" = 2 (ocrs_engine_set_option).  For a 3x3 conv with
 * the n_w weights w, the n_bias biases and a fused ReLU or none, and a 4 x 32 patch at image row y0 of an image h rows high
 * (both multiples of 4) with cin input channels (a multiple of 32):
 *   out[0]      1 = dropping the matrix-core work of tap rows outside the image changes no bit of this layer's output
 *               (every weight finite, and a ReLU follows or no bias is -0.0), 0 = the layer keeps that work
 *   out[1..2]   the K loop's 16-deep chunks [0, out[1]) leave out patch row 0, chunks [out[2], 9 cin / 16) patch row 3
 *   out[3..5]   per phase of the K loop (taps 0..2, 3..5, 6..8): the patch row that is left out, -1 = none.
 * With out[0] = 0 nothing is left out. */
OCRS_API ocrs_status ocrs_conv_rows_selftest(const float* w, size_t n_w, const float* bias, size_t n_bias, int relu, int y0, int h,
                                             int cin, int32_t out[6]);

/* Integer tuning options (no reference counterpart: RTen's equivalents are compile-time).  They select between kernels
 * that compute the SAME bits — results never depend on an option; the tests run the alternatives against each other.
 *
 * Scope.  The process holds the defaults: initial value from the environment variable OCRS_<NAME IN CAPITALS>, read once
 * when the library first needs an option; ocrs_set_option changes a default.  An engine COPIES the defaults when it is
 * created (ocrs_engine_new / ocrs_engine_group_new) and from then on owns its copy: ocrs_engine_set_option changes one
 * engine only, two engines in one process can differ, and changing a default never affects an engine that exists.
 * ocrs_model_run on a bare model uses the defaults.  Set an engine's options before it is in use by other threads.
 *
 *   "gru_mode"        0 = one persistent kernel per GRU layer (default), 1 = one launch per time step
 *   "gru_gates"       1 = requests small enough that every 16-line row tile gets its own cluster of workgroups run the
 *                     gate-per-wave recurrence kernel (default), 0 = always the general persistent kernel (exact numerics
 *                     only: the relaxed / reduced modes have one persistent recurrence kernel for every request size)
 *   "gru_local"       persistent GRU kernels: 1 = a cluster of workgroups that finds itself on one XCD hands its state
 *                     over through that XCD's L2 (default), 0 = always through write-through stores
 *   "det_fuse"        1 = fused DoubleConv blocks of the detection U-Net for every block shape that has a fused kernel
 *                     (default; 2 = the same, kept for older callers), 0 = per-operator kernels only
 *   "det_stream"      1 (default) = the DoubleConv blocks of the U-Net's full-resolution level run as row-streaming wave
 *                     kernels (a wave walks down a 64-column strip, a lane keeps its pixel's channels in registers,
 *                     horizontal taps through DPP lane shifts), rows per wave chosen from the request's size; 8 / 14 / 32 =
 *                     the same with that many rows per wave; 0 = the LDS-tiled blocks
 *   "det_rows"        1 (default) = the DoubleConv blocks of the 16-64-channel levels run as row-streaming workgroup
 *                     kernels for requests of up to 8 pages; 8 / 14 / 20 / 32 = those kernels for every request, with that
 *                     many rows per workgroup; 0 = the LDS-tiled blocks always
 *   "ccl_quad"        1 (default) = the component-labelling and root-compaction kernels of detect_words handle four mask
 *                     pixels per thread when the page width is a multiple of 4; 0 = one pixel per thread
 *   "conv12_fuse"     1 (default) = the first two recognition convs and their 2x2 pools run as one kernel (conv1 into an
 *                     LDS tile per patch, conv2's matrix-core loop reads its operand there); 0 = two kernels
 *   "conv_flat"       recognition 3x3 convs: the 128-pixel patches tile a width group's strip of images side by side
 *                     (1, default: only a group's last patch is ragged) or every image on its own (0)
 *   "beam_gpu"        1 = DecodeMethod::BeamSearch runs on the GPU (default), 0 = on the host (threaded over lines)
 *   "det_tile_batch"  tiled detection (ocrs_engine_detect_words_tiled ...): tiles per run of the detection model, 1 .. 1024
 *                     (default 16); bounds the activation memory of a request whatever its page sizes, never changes a result
 *   "stream_budget"   streams a device uses, 3 .. 16 (default 4, the hardware queues the runtime opens by default): one for
 *                     the recognition conv stacks, one for the recurrences, the rest shared by everything else of all calls
 *                     in flight, each call on the least loaded; 0 = a stream per call in flight, as before this option.  A
 *                     device's plan serves every engine on it: a process option only (ocrs_engine_set_option refuses it),
 *                     taken up by a device between calls, and OCRS_ERR_INVALID_ARGUMENT while a call is in flight on one
 *
 * OCRS_ERR_INVALID_ARGUMENT for an unknown name.  (Rounds 2-4 carried 28 process-wide options, many of them switches for
 * experiments that had lost their A/B; round 5 removed those kernels and moved what is configuration — numerics, request
 * coalescing, host threads, the sub-request size, the group's dealing blocks — into ocrs_engine_params / ocrs_group_params.) */
OCRS_API ocrs_status ocrs_set_option(const char* name, long value);
/* Name of option `index` (0 .. count - 1); *name = NULL past the last one. */
OCRS_API ocrs_status ocrs_option_name(int index, const char** name);

/* Memory the library holds on a device: out = {device bytes in use, device bytes cached (free, reusable), cap on the
 * cached device bytes, peak of bytes in use, hipMalloc calls, blocks returned to the driver, and the same six numbers for
 * the pinned host staging pool of that device's context}.  device < 0: the default device. */
OCRS_API ocrs_status ocrs_device_pool_stats(int device, uint64_t out[12]);
/* Caps on the CACHED bytes (0 = leave as is).  Defaults: a quarter of the device's memory (environment variable
 * OCRS_POOL_CAP_GB, read once per device, overrides) and 1 GiB of pinned host memory.  Blocks above a cap are returned
 * to the driver by a background thread, never on a request's thread (hipFree waits for the device). */
OCRS_API ocrs_status ocrs_device_pool_configure(int device, uint64_t device_cached_cap_bytes, uint64_t pinned_cached_cap_bytes);
/* Gives back what the library holds for re-use on `device`: every cached block and the activation arena the recognition conv
 * stacks of all requests share (kept at the size of the largest request seen).  Bytes in use afterwards = weights, pages the
 * caller still holds, requests in flight.  Waits for the conv stacks in flight; for idle moments, not for the request path. */
OCRS_API ocrs_status ocrs_device_pool_trim(int device);

/* Isolation of the bf16-MFMA kernels (engines with numerics != exact), per device.  Round 5 observed OTHER requests' line crops
 * change while those kernels ran beside them; round 6 reproduced it from the two real kernels alone (tools/hazard_repro.hip:
 * every twin launch of the crop kernel differs while a dense bf16-MFMA kernel whose matrix instructions read VGPR operands shares its compute units,
 * none when the two are confined to disjoint units; DESIGN.md §4.4 "Concurrency").  The library therefore never lets kernels of
 * different requests overlap on a device that has such an engine.
 *   OCRS_ISOLATION_AUTO (default)   every call on the device enqueues on ONE stream while such an engine exists;
 *   OCRS_ISOLATION_NONE             nothing (diagnostics: tools/hazard_canary.py reproduces the hazard with it — never in
 *                                   production).
 * Exact-only devices are untouched by any of this (and covered by a standing canary: tests/test_gpu_r6.py).  A request is told
 * its regime once, when it starts, and keeps it; a change of regime — this call, the first engine with numerics != exact
 * created on the device, the last one destroyed — BLOCKS until the requests in flight on the device have finished (new ones
 * wait meanwhile) and the device is idle, so requests of two regimes never run side by side.  Do not call from inside a
 * request.  device < 0: the default device. */
typedef enum { OCRS_ISOLATION_AUTO = 0, OCRS_ISOLATION_NONE = 1 } ocrs_isolation;
OCRS_API ocrs_status ocrs_device_set_isolation(int device, ocrs_isolation policy);
/* out = {what a request starting now is told: 0 free (the lanes of option "stream_budget"), 1 serial (one stream);
 *        engines with numerics != exact alive on the device; compute units of the device}. */
OCRS_API ocrs_status ocrs_device_isolation(int device, int out[3]);

/* ------------------------------------------------------------------------
 * L2 seam: `trait Model` (ocrs/src/model.rs:6-17) and its rten impl
 * (model.rs:19-41).  A Rust `impl Model for HipModel` binds these four calls
 * (INTEGRATION.md §1).
 * ---------------------------------------------------------------------- */
typedef struct ocrs_model ocrs_model;

/* rten::Model::load_file (ocrs-cli/src/models.rs:100-107): loads an `.ocrsm`
 * fixed-graph file and uploads the weights to HBM. */
OCRS_API ocrs_status ocrs_model_load_file(const char* path, ocrs_model** out);
OCRS_API ocrs_status ocrs_model_load_bytes(const void* data, size_t len, ocrs_model** out);
/* The same with the weights on an explicit device (device < 0: the default device).  The file is validated on the
 * host first; a malformed file fails with OCRS_ERR_IO before any device is touched. */
OCRS_API ocrs_status ocrs_model_load_file_on_device(const char* path, int device, ocrs_model** out);
OCRS_API ocrs_status ocrs_model_load_bytes_on_device(const void* data, size_t len, int device, ocrs_model** out);
/* Device that holds the model's weights (-1 for a callback model). */
OCRS_API ocrs_status ocrs_model_device(const ocrs_model* m, int* device);

/* A model implemented by the caller — the counterpart of implementing
 * `trait Model` in Rust (the reference's tests inject FakeDetectionModel /
 * FakeRecognitionModel this way, lib.rs:339-422).  `run` receives a contiguous
 * NCHW f32 input, must malloc() the output, fill out_shape/out_ndim (<= 4) and
 * return 0; non-zero means failure (-> OCRS_ERR_RUN_FAILED). */
typedef int (*ocrs_model_run_fn)(void* user, const float* input, const int64_t in_shape[4], float** output,
                                 int64_t out_shape[4], int* out_ndim);
OCRS_API ocrs_status ocrs_model_from_callback(const int64_t input_shape[4], /* -1 = symbolic */
                                     ocrs_model_run_fn run, void* user, ocrs_model** out);

/* Model::input_shape (model.rs:20-31): NCHW; dims[i] = -1 and is_fixed[i] = 0
 * for Dimension::Symbolic. */
OCRS_API ocrs_status ocrs_model_input_shape(const ocrs_model* m, int64_t dims[4], uint8_t is_fixed[4]);

typedef struct ocrs_run_options {
    int timing; /* RunOptions.timing (detection.rs:178-182): print per-op times */
} ocrs_run_options;

/* Model::run (model.rs:33-40).  `input` is host memory, contiguous NCHW f32.
 * Detection graphs return [N,1,H,W] probabilities; recognition graphs return
 * [T,N,C] log-probabilities (recognition.rs:399-401).  *output is host memory
 * owned by the caller (ocrs_buffer_free). */
OCRS_API ocrs_status ocrs_model_run(const ocrs_model* m, const float* input, const int64_t in_shape[4],
                           const ocrs_run_options* opts, float** output, int64_t out_shape[4], int* out_ndim);

/* Algorithmic FLOPs of one forward at the given input shape. */
OCRS_API ocrs_status ocrs_model_flops(const ocrs_model* m, const int64_t in_shape[4], double* flops);

OCRS_API void ocrs_model_free(ocrs_model* m);

/* ------------------------------------------------------------------------
 * L4 API: OcrEngine (ocrs/src/lib.rs:111-301) with the grey page resident in
 * HBM between calls (OcrInput, lib.rs:125-128).
 * ---------------------------------------------------------------------- */
typedef struct ocrs_engine ocrs_engine;
typedef struct ocrs_page ocrs_page; /* OcrInput */

typedef enum ocrs_numerics { OCRS_NUMERICS_EXACT = 0, OCRS_NUMERICS_RELAXED = 1, OCRS_NUMERICS_REDUCED = 2 } ocrs_numerics;

typedef enum ocrs_decode_method { /* DecodeMethod, recognition.rs:198-205 */
    OCRS_DECODE_GREEDY = 0,
    OCRS_DECODE_BEAM_SEARCH = 1
} ocrs_decode_method;

/* OcrEngineParams (lib.rs:38-71).  Models are borrowed: they must outlive the
 * engine.  NULL strings select the defaults (DEFAULT_ALPHABET, lib.rs:34). */
typedef struct ocrs_engine_params {
    const ocrs_model* detection_model;   /* may be NULL */
    const ocrs_model* recognition_model; /* may be NULL */
    int debug;
    ocrs_decode_method decode_method;
    uint32_t beam_width;
    const char* alphabet;      /* UTF-8 */
    const char* allowed_chars; /* UTF-8 */
    /* --- no reference counterpart (RTen is fp32 on the CPU, one page per call) --- */
    ocrs_numerics numerics;    /* OCRS_NUMERICS_EXACT (0, default): every kernel follows the numeric spec, results are
                                * bit-identical to the CPU oracle.  The other two are EXPERIMENTAL.  OCRS_NUMERICS_RELAXED: fp32-class arithmetic that is not
                                * reproducible on a CPU — hardware exp / rcp in the recurrence's gates; the operands of the
                                * recognition convs, the GRU input projections and the recurrence's own contraction cut
                                * into three bf16 terms on the bf16 matrix cores (products good to 2^-23), the matrix core's
                                * accumulation order.  OCRS_NUMERICS_REDUCED: the same with two bf16 terms per
                                * operand (products good to 2^-15: a 16-bit significand).  Boxes and tokens are expected, not
                                * guaranteed, to match the exact mode: DESIGN.md "what exactness costs" has the measured flips.
                                * While an engine of these modes exists, every call on its device (of any engine of the
                                * process) runs its kernels one at a time on one stream (ocrs_device_set_isolation below says why and what a
                                * change of regime waits for): create it before serving traffic */
    int coalesce;              /* one-page calls that wait at the same time are merged into one ragged request per stage
                                * (lines are independent: nobody's bits change).  Merged batches in flight per stage:
                                * 0 = default (2), negative = every call runs on its own */
    int coalesce_pages;        /* pages per merged batch (0 = default 16); requests of half that size or more are never merged */
    int coalesce_window_us;    /* while other batches are in flight, how long the next one lets its queue fill
                                * (0 = default 300, negative = no wait) */
    int layout_threads;        /* host threads ocrs_engine_find_text_lines_batch may use (0 = one per page up to the host's cores) */
    int64_t rec_max_pixels;    /* input pixels (padded line batch) one recognition sub-request may hold; larger requests run
                                * as consecutive sub-requests (0 = 2e9, sized for the activation memory of one GPU) */
} ocrs_engine_params;

/* OcrEngine::new (lib.rs:132-180).  The engine lives on its models' device (both models must be on the same one;
 * an engine with callback models only lives on the default device); pages it prepares live there too, and a page
 * can only be given to an engine of its own device (OCRS_ERR_INVALID_ARGUMENT otherwise). */
OCRS_API ocrs_status ocrs_engine_new(const ocrs_engine_params* params, ocrs_engine** out);
OCRS_API void ocrs_engine_free(ocrs_engine* e);
OCRS_API ocrs_status ocrs_engine_device(const ocrs_engine* e, int* device);
/* This engine's copy of a tuning option (see ocrs_set_option for the list and the scoping rule).  Also accepted, by
 * field name: "coalesce", "coalesce_pages", "coalesce_window_us", "layout_threads", "rec_max_pixels" (the values as
 * stored: coalesce 0 = off); "numerics" can be read but is fixed when the engine is created.
 * One more name belongs to an engine alone (no process default, no environment variable, not listed by ocrs_option_name):
 *   "conv_rows"       exact recognition 3x3 convs with 128-column blocks (Cout a multiple of 128, image height a multiple of 4);
 *                     the same bits at every value.  2 (every new engine's value) = each of a block's four waves owns all four
 *                     image rows of a 4 x 32 patch and a quarter of the columns, and where the model allows (every weight
 *                     finite; a ReLU behind the conv or no -0.0 bias) the rows above and below the image cost no matrix-core
 *                     work; 1 = the same waves, every multiplication kept; 0 = blocks of 2 x 2 waves */
OCRS_API ocrs_status ocrs_engine_set_option(ocrs_engine* e, const char* name, long value);
OCRS_API ocrs_status ocrs_engine_get_option(const ocrs_engine* e, const char* name, long* value);

typedef enum ocrs_dim_order { OCRS_HWC = 0, OCRS_CHW = 1 } ocrs_dim_order; /* DimOrder, preprocess.rs:50-57 */
typedef enum ocrs_pixel_type { OCRS_U8 = 0, OCRS_F32 = 1 } ocrs_pixel_type; /* ImagePixels, preprocess.rs:9-14 */

/* ImageSource::from_bytes (preprocess.rs:81-101): validates only. */
OCRS_API ocrs_status ocrs_image_source_check_bytes(size_t len, uint32_t width, uint32_t height, uint32_t* channels);

/* ImageSource::from_tensor + OcrEngine::prepare_input (preprocess.rs:105-123,
 * lib.rs:183-187): converts to greyscale f32 [1,H,W] in [-0.5,0.5] on the GPU.
 * `pixels` is host memory. */
OCRS_API ocrs_status ocrs_engine_prepare_input(const ocrs_engine* e, const void* pixels, ocrs_pixel_type type,
                                      ocrs_dim_order order, int height, int width, int channels,
                                      ocrs_page** out);
/* Several equally sized host images in one call: all uploads and conversions are queued on one stream and waited
 * for once (OcrEngine::prepare_input, lib.rs:183-187, per image).  out[n] receives the pages.  The form bench.py's
 * headline times (host pixels in page-locked buffers, the upload inside the timed region). */
OCRS_API ocrs_status ocrs_engine_prepare_input_batch(const ocrs_engine* e, const void* const* pixels, size_t n,
                                                     ocrs_pixel_type type, ocrs_dim_order order, int height, int width,
                                                     int channels, ocrs_page** out);
/* Same, with `pixels` already resident in HBM (device pointer): what a GPU image decoder hands over (bench.py
 * --resident and its `value_resident` extra time this form). */
OCRS_API ocrs_status ocrs_engine_prepare_input_device(const ocrs_engine* e, const void* d_pixels, ocrs_pixel_type type,
                                             ocrs_dim_order order, int height, int width, int channels,
                                             ocrs_page** out);
OCRS_API void ocrs_page_free(ocrs_page* p);
OCRS_API ocrs_status ocrs_page_dims(const ocrs_page* p, int* height, int* width);
/* Copy the prepared grey page [H,W] f32 to host (OcrInput.image, lib.rs:127). */
OCRS_API ocrs_status ocrs_page_image(const ocrs_page* p, float* out_hw);
/* The inverse of ocrs_page_image: a page on the engine's device from an already prepared grey image [H,W] f32 (host
 * memory), copied bit for bit; nothing is converted or checked.  For a caller that keeps prepared pages on the host. */
OCRS_API ocrs_status ocrs_engine_page_from_grey(const ocrs_engine* e, const float* grey_hw, int height, int width, ocrs_page** out);

/* OcrEngine::detect_words (lib.rs:193-199 -> detection.rs:104-122).
 * *rects receives n x 6 floats in contour discovery order. */
OCRS_API ocrs_status ocrs_engine_detect_words(const ocrs_engine* e, const ocrs_page* page, float** rects, size_t* n);
/* Batched form: pages of ANY sizes (the reference takes any image per call, detection.rs:131-171; the model runs once over
 * the whole batch at its own fixed size, the size-dependent kernels once per distinct page size — r6; rounds 1-5 wanted one
 * size per batch); rects of page i are (*rects)[6*offsets[i] .. 6*offsets[i+1]); offsets has n_pages+1 entries.  Concurrent
 * one-page calls are merged the same way whatever their sizes. */
OCRS_API ocrs_status ocrs_engine_detect_words_batch(const ocrs_engine* e, const ocrs_page* const* pages, size_t n_pages,
                                           float** rects, size_t* offsets);

/* Detection confidence: the two calls above, plus, per returned rect and indexed like the rects,
 *   pixels: the number of text-mask pixels of the word's connected component (8-connected foreground; holes and what lies
 *           inside them do not count);
 *   score:  the mean text probability of those pixels, computed from an integer sum so that it never depends on batching
 *           or scheduling: (float)(sum of floor(clamp(p, 0, 1) * 2^24) / (pixels * 2^24)), p from the map
 *           ocrs_engine_detect_text_pixels returns.  The fixed point costs less than 2^-24 a pixel; at most 1.
 * Both malloc'ed (ocrs_buffer_free).  The rects are those of the unscored calls.  Filtering by score is the caller's: there
 * is no engine option for it.  Scores say how sure the model was, not whether it is right: calibrate on real models before
 * thresholding. */
OCRS_API ocrs_status ocrs_engine_detect_words_scored(const ocrs_engine* e, const ocrs_page* page, float** rects, size_t* n,
                                                     float** score, uint32_t** pixels);
OCRS_API ocrs_status ocrs_engine_detect_words_batch_scored(const ocrs_engine* e, const ocrs_page* const* pages, size_t n_pages,
                                                           float** rects, size_t* offsets, float** score, uint32_t** pixels);

/* OcrEngine::detect_text_pixels (lib.rs:207-213 -> detection.rs:131-200):
 * writes the [H,W] probability map. */
OCRS_API ocrs_status ocrs_engine_detect_text_pixels(const ocrs_engine* e, const ocrs_page* page, float* out_hw);

/* Tiled detection, opt-in per call: a page larger than the detection model's input Hm x Wm is not squeezed
 * into it but cut into Hm x Wm tiles at its own resolution; the tiles run through the model as a batch (about one detector
 * run per tile) and every page pixel takes its probability from the one tile that owns it.  From that map on the call is the
 * untiled one.  Along an axis of page length L and model length M, with overlap v (0 <= v <= min(Hm, Wm) / 2, integer
 * arithmetic): L <= M: one tile at 0 owning [0, L).  Else n = ceil((L - v) / (M - v)) tiles at o_i = (i * (L - M)) / (n - 1),
 * tile i owning [b_i, b_i+1) with b_0 = 0, b_n = L, b_i = (o_i-1 + M + o_i) / 2.  Tiles of a page: rows x columns, row-major.
 * A tile's input is the page cut at its origin, -0.5 where it reaches past the page; nothing is ever resized.  A page no
 * larger than the model input has one tile and the results of the untiled call, bit for bit.  A page's result never depends
 * on the rest of the batch or on "det_tile_batch".
 * overlap: pixels; negative = OCRS_TILE_OVERLAP_DEFAULT (a value chosen on synthetic weights, not a claim about real
 * models); beyond min(Hm, Wm) / 2: OCRS_ERR_INVALID_ARGUMENT.  Tiled requests are never merged with concurrent requests.
 * A caller-implemented model (ocrs_model_from_callback) is run once per tile, in tile order within the caller's page order.
 *
 * ocrs_detection_tile_plan: the plan the engine uses (host only, no GPU): *ny x *nx tiles; origin_y [ny], bound_y [ny + 1],
 * origin_x [nx], bound_x [nx + 1], malloc'ed int32 (ocrs_buffer_free). */
#define OCRS_TILE_OVERLAP_DEFAULT 100
OCRS_API ocrs_status ocrs_detection_tile_plan(int page_h, int page_w, int model_h, int model_w, int overlap, size_t* ny, size_t* nx,
                                              int32_t** origin_y, int32_t** bound_y, int32_t** origin_x, int32_t** bound_x);
/* Output as ocrs_engine_detect_words[_batch]_scored; score and pixels may BOTH be NULL (then nothing extra is allocated or
 * launched, as in the unscored calls). */
OCRS_API ocrs_status ocrs_engine_detect_words_tiled(const ocrs_engine* e, const ocrs_page* page, int overlap, float** rects, size_t* n,
                                                    float** score, uint32_t** pixels);
OCRS_API ocrs_status ocrs_engine_detect_words_batch_tiled(const ocrs_engine* e, const ocrs_page* const* pages, size_t n_pages, int overlap,
                                                          float** rects, size_t* offsets, float** score, uint32_t** pixels);
/* The stitched [H,W] probability map of the tiled call. */
OCRS_API ocrs_status ocrs_engine_detect_text_pixels_tiled(const ocrs_engine* e, const ocrs_page* page, int overlap, float* out_hw);

/* ------------------------------------------------------------------------
 * Working resolution (no reference counterpart, opt-in).  The plain detection call squeezes any page into the
 * model input with one bilinear resize; the tiled call never resizes.  These calls let the caller choose the resolution the
 * detector sees: a resident page is resampled on the device to a work size, detection runs on that work page (plain or
 * tiled), and the word rects come back in the frame of the page as given, so that layout and recognition run on the
 * full-resolution page.  A resampled page is an ordinary ocrs_page: every other call takes it.
 *
 * ocrs_engine_resize_page[s]: *out = the page resampled to out_h x out_w (each 1 .. 65535, as are the page's own sides;
 * else OCRS_ERR_INVALID_ARGUMENT), a new page on the page's device, independent of the source; release both with
 * ocrs_page_free in any order.  The batch form serves n pages of any sizes, each to its own out_hw[2i], out_hw[2i+1] with its
 * own filters[i], in one launch; out[n] receives the pages.  float32 arithmetic, every operation rounded on its own:
 *   OCRS_RESAMPLE_BILINEAR  any sizes: the bilinear resize of the detection path (ONNX Resize linear / half_pixel) on the
 *                           page itself, no padding.
 *   OCRS_RESAMPLE_AREA      out_h <= H and out_w <= W (else OCRS_ERR_INVALID_ARGUMENT): the exact area average.  Along one
 *                           axis L -> l: g = gcd(L, l), P = L / g, q = l / g; output j covers [jP, (j+1)P), source x covers
 *                           [xq, (x+1)q); taps x = (jP) / q .. ((j+1)P - 1) / q ascending, each with the integer weight
 *                           ov = min((j+1)P, (x+1)q) - max(jP, xq); acc = float(ov0) * in[x0], acc = acc + float(ov) * in[x],
 *                           value = acc / float(P).  Horizontally per source row of the vertical footprint, then the same
 *                           rule vertically over those values.  Equal sizes: the identity; a halving: ((a+b)/2 + (c+d)/2)/2.
 *   OCRS_RESAMPLE_AUTO      area when neither side grows, else bilinear.
 *
 * ocrs_work_size (host only): the work size of a scale: h = clamp((int)floor(page_h * scale + 0.5), 1, 65535) in double, w
 * likewise.  A scale that is not finite or not positive: OCRS_ERR_INVALID_ARGUMENT.
 *
 * ocrs_rescale_rects (host only, in place): rects of the from_h x from_w frame of a picture in its to_h x to_w frame.
 * Coordinates are points of the pixel-index frame (pixel i covers [i - 0.5, i + 0.5)).  Equal sizes leave every bit as it
 * is.  Otherwise, in double from the float32 values, each operation as written, the results rounded to float32:
 * sx = to_w / from_w, sy = to_h / from_h; cx' = (cx + 0.5) * sx - 0.5, cy' likewise with sy; v = (up.x * sx, up.y * sy),
 * lv = sqrt(v.x^2 + v.y^2); a = (-up.y * sx, up.x * sy), la = sqrt(a.x^2 + a.y^2); lv finite and > 0: up' = v / lv,
 * h' = h * lv, w' = w * la; otherwise up stays, h' = h * sy, w' = w * sx.  An axis-aligned rect is mapped exactly; a tilted
 * one under sx != sy (the rounding of a work size: under one pixel over the page) within that relative error.
 *
 * ocrs_engine_detect_words[_batch]_at: detection at a work size per page, work_hw[2i], work_hw[2i+1]; 0, 0 = the page's own
 * size.  (1) The pages whose work size differs from their own are resampled with `filter` in one launch; (2) the work pages
 * go through detection as the pages of ocrs_engine_detect_words_batch do (tiled == 0; may be merged with concurrent
 * requests) or those of ocrs_engine_detect_words_batch_tiled (tiled != 0, overlap as there); (3) the rects return in each
 * page's own frame through ocrs_rescale_rects.  score and pixels (both or neither; may be NULL) are those of the WORK page
 * (§7.1), and the reference's 3-pixel pad of a word box and its area >= 100 rule apply at work resolution, before the map.
 * A page whose work size is its own is not resampled and has the plain (or tiled) call's bits.  Outputs as
 * ocrs_engine_detect_words_batch_scored. */
typedef enum ocrs_resample_filter { OCRS_RESAMPLE_AUTO = 0, OCRS_RESAMPLE_BILINEAR = 1, OCRS_RESAMPLE_AREA = 2 } ocrs_resample_filter;
OCRS_API ocrs_status ocrs_engine_resize_page(const ocrs_engine* e, const ocrs_page* page, int out_h, int out_w, int filter, ocrs_page** out);
OCRS_API ocrs_status ocrs_engine_resize_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* out_hw,
                                              const int* filters, ocrs_page** out);
OCRS_API ocrs_status ocrs_work_size(int page_h, int page_w, double scale, int* h, int* w);
OCRS_API ocrs_status ocrs_rescale_rects(float* rects6, size_t n, int from_h, int from_w, int to_h, int to_w);
OCRS_API ocrs_status ocrs_engine_detect_words_at(const ocrs_engine* e, const ocrs_page* page, int work_h, int work_w, int filter, int tiled,
                                                 int overlap, float** rects, size_t* n, float** score, uint32_t** pixels);
OCRS_API ocrs_status ocrs_engine_detect_words_batch_at(const ocrs_engine* e, const ocrs_page* const* pages, size_t n_pages,
                                                       const int* work_hw, int filter, int tiled, int overlap, float** rects,
                                                       size_t* offsets, float** score, uint32_t** pixels);

/* ------------------------------------------------------------------------
 * Page normalisation (no reference counterpart, opt-in).  What rotate and resize do to a page's geometry,
 * this does to its grey levels: a phone photo with a shadow across it, a faint photocopy or a dark-mode screenshot becomes
 * a new resident page with ink at -0.5 and paper at +0.5, dark text on a light page whatever came in, and every other
 * call takes that page.  Coordinates do not move, so nothing needs mapping back.  The source page is untouched; release
 * both with ocrs_page_free in any order.  What a trained detector gains is uncalibrated: the figures of DESIGN.md §7.4
 * are for the synthetic detection files only.
 *
 * The definition (tests/normalize_ref.py restates it and the library equals it bit for bit; float32, every operation
 * rounded on its own; all counting in integers, so the result does not depend on schedule or batch):
 *   bins      g = clamp(v + 0.5f, 0, 1), NaN stays NaN and is not counted; bin = floor(g * 256f) kept within 0 .. 255.
 *             Tiles are tile x tile pixels from the page origin, edge tiles partial.  pct(h, num, den) = the smallest bin
 *             whose cumulative count c has c * den >= num * n; -1 for an empty histogram.
 *   polarity  AUTO: every non-empty tile adds pct(19,20) + pct(1,20) - 2 pct(1,2) of its histogram to a vote (does the
 *             tile's median sit nearer its dark or its bright end, weighted by the tile's contrast); the page is dark iff
 *             the vote > 0.  KEEP: light, INVERT: dark; the vote stays 0.  On a dark page g = clamp(0.5f - v, 0, 1)
 *             and the tile and page histograms are read mirrored (bin 255 - b).
 *   flatten   white bin of a tile = pct(3,4) of its effective histogram, Wg = the same of the page's.  A present tile's
 *             value is max(white, Wg / 2) (a tile inside a dark figure is not blown up to white), then the maximum over
 *             the present tiles of its 3 x 3 neighbourhood (a heading that fills a tile is not read as background); an
 *             empty tile takes max(Wg, 0).  Level L = (bin + 1) / 256.  B = L interpolated bilinearly over tile centres:
 *             fy = (y + 0.5f) * (1 / tile) - 0.5f kept within [0, tiles_y - 1], x likewise, top = (1 - wx) L00 + wx L01,
 *             bot likewise, B = (1 - wy) top + wy bot.  u = min(g / B, 1).  flatten == 0: u = g.
 *   levels    histogram of u over the page, binned as above; lo = pct(1,100), hi = pct(1,2) (the median is the paper).
 *             hi > lo >= 0: out = clamp((u - lo/256) / (hi/256 - lo/256), 0, 1) - 0.5f; otherwise (a blank page, an
 *             all-NaN page) and with levels == 0: out = u - 0.5f.
 *   neither   flatten == 0 and levels == 0: the page's own 32-bit words, the sign bit flipped on a dark page.
 * NaN stays NaN and only NaN does; with flatten or levels on, every other result lies in [-0.5, 0.5].
 *
 * ocrs_normalize_params_default: tile 64, OCRS_POLARITY_AUTO, flatten 1, levels 1.  ocrs_normalize_params_check (host
 * only): OCRS_ERR_INVALID_ARGUMENT for a tile that is not a power of two in 16 .. 256 or an unknown polarity; the engine
 * calls refuse the same, and a page with a side over 65535.  ocrs_engine_normalize_pages serves n pages of any sizes, each
 * with its own params[i], in five launches for the whole batch on one stream; out_pages[n] receives the pages, out_info[n]
 * (may be NULL) what was found.  ocrs_engine_normalize_page: params == NULL means the default. */
typedef enum ocrs_polarity { OCRS_POLARITY_AUTO = 0, OCRS_POLARITY_KEEP = 1, OCRS_POLARITY_INVERT = 2 } ocrs_polarity;
typedef struct ocrs_normalize_params {
    int32_t tile;     /* a power of two, 16 .. 256 */
    int32_t polarity; /* ocrs_polarity */
    int32_t flatten;  /* 0 / 1 */
    int32_t levels;   /* 0 / 1 */
} ocrs_normalize_params;
typedef struct ocrs_normalize_info {
    int32_t dark;     /* 1: the page was read as light text on a dark page and inverted */
    int32_t white;    /* Wg; -1: no pixel was counted */
    int32_t lo, hi;   /* the bins of u the levels were taken from; -1, -1 with levels == 0 or nothing counted */
    int64_t vote;     /* the polarity vote; 0 unless OCRS_POLARITY_AUTO */
    uint64_t counted; /* pixels that are not NaN */
} ocrs_normalize_info;
OCRS_API ocrs_status ocrs_normalize_params_default(ocrs_normalize_params* out);
OCRS_API ocrs_status ocrs_normalize_params_check(const ocrs_normalize_params* params);
OCRS_API ocrs_status ocrs_engine_normalize_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_normalize_params* params,
                                                ocrs_page** out_page, ocrs_normalize_info* out_info);
OCRS_API ocrs_status ocrs_engine_normalize_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                                 const ocrs_normalize_params* params, ocrs_page** out_pages, ocrs_normalize_info* out_info);

/* ------------------------------------------------------------------------
 * Page deskew (no reference counterpart, opt-in).  A page that went through the feeder a few degrees off
 * breaks find_text_lines' grouping before the rectified crops (§8.4) can help.  These calls measure the skew of a resident
 * page without a detector and without knowing its polarity, make the upright page as a new resident page, and map what was
 * found on it back to the frame of the scan.  tests/deskew_ref.py restates every definition; the library equals it bit for
 * bit (the trigonometry of ocrs_skew_table and ocrs_deskew_map is libm's: held within one unit of the last place).
 *
 * ocrs_engine_skew_scores: out_scores[i * n_angles + a] = the profile score of page i at angle a, for n pages of any sizes
 * in one launch (plus one small launch that squares and sums).  sc_table[2a], sc_table[2a + 1] = S, C = the angle's sine
 * and cosine in Q16 (round(sin * 65536)); the caller makes the table (ocrs_skew_table), so the result is integer arithmetic
 * throughout and does not depend on schedule, batch or launch shape.  For a page of H x W:
 *   q(x, y)   the bin of Page normalisation above: g = clamp(v + 0.5f, 0, 1), floor(g * 256f) kept within 0 .. 255
 *   d(x, y)   |q(x, y) - q(x, y + 1)| for y < H - 1; 0 on the last row and when either pixel is NaN.  A vertical
 *             difference is polarity-free, and flat paper weighs nothing, so the varying length of a projection row needs
 *             no correction
 *   bin       (x S + y C - t0) >> 16, t0 = min(0, (W - 1) S) + min(0, (H - 1) C) (the minimum over the four corners)
 *   P[b]      the sum of d over the pixels of bin b (uint32);  score = sum over b of P[b]^2 (uint64)
 * y points down: a page whose content was turned counter-clockwise by t (PIL's rotate(t)) has baselines along
 * (cos t, -sin t), constant in x sin t + y cos t, so the score peaks at +t.  OCRS_ERR_INVALID_ARGUMENT for n_angles < 1
 * (or > 65535), an |S| or |C| above 65536, and a page side above 4096 (x S + y C - t0 must stay inside int32: the
 * estimate is meant for a work copy); OCRS_ERR_CAPACITY for more than 65535 pages or more than 2 GiB of profiles
 * (4 n_angles (H + W) bytes per page) in one call.
 *
 * ocrs_skew_table (host only): sc_table[2i], [2i + 1] = S, C of the angle (first + i) * step_deg degrees, i < n:
 * round-to-nearest-even of sin / cos (double, libm) * 65536.
 *
 * ocrs_engine_estimate_skew: (1) a page whose longer side exceeds work_max_side is shrunk with OCRS_RESAMPLE_AREA to
 * ocrs_work_size(scale = work_max_side / longer side); a smaller page goes as it is; (2) the scores of the coarse angles
 * k r * fine_step_deg, k = -K .. K, r = coarse_step_deg / fine_step_deg (a whole number), K = floor(max_deg /
 * coarse_step_deg); (3) the scores of the 2 r + 1 angles one fine step apart around the best coarse one; (4) the arg max,
 * on the host.  Every angle is an integer multiple of the fine step; ties go to the smaller |angle|, then to the negative
 * one, so a blank page has angle 0.  params == NULL: ocrs_skew_params_default (work_max_side 1024, max_deg 15, coarse 0.5,
 * fine 0.1).  ocrs_skew_params_check (host only) refuses work_max_side outside 1 .. 4096, max_deg outside (0, 45], steps
 * that are not positive or whose ratio is not whole, and fewer than one coarse step.
 *
 * ocrs_engine_warp_page[s]: *out = a new out_h x out_w page (sides 1 .. 65535), independent of its source; release both
 * with ocrs_page_free in any order.  The batch form serves n pages of any sizes, each with its own out_hw[2i], [2i + 1],
 * m[6i .. 6i + 5] and fill[i], in one launch.  float32, every operation rounded on its own (§8.4's expression form):
 * fx = ox + 0.5f, fy = oy + 0.5f; X = (m0 + m1 fx) + m2 fy, Y = (m3 + m4 fx) + m5 fy; ix = floor(X), wx = X - ix, y
 * likewise; taps (ix, iy) .. (ix + 1, iy + 1), a tap outside the page is `fill`; top = (1 - wx) t00 + wx t01, bot likewise,
 * v = (1 - wy) top + wy bot.  Coefficients that are not finite: OCRS_ERR_INVALID_ARGUMENT.
 *
 * ocrs_deskew_map (host only): the map that undoes a skew of +angle_deg (|angle| <= 45, else OCRS_ERR_INVALID_ARGUMENT):
 * the output is the page turned clockwise by t about its centre.  In double, each coefficient rounded once to float32:
 * W' = ceil(w |cos t| + h |sin t|), H' = ceil(w |sin t| + h |cos t|) when expand, else W' = w, H' = h;  m1 = cos t,
 * m2 = sin t, m0 = (w/2 - 0.5) - cos t W'/2 - sin t H'/2;  m4 = -sin t, m5 = cos t, m3 = (h/2 - 0.5) + sin t W'/2 -
 * cos t H'/2.  out_hw = {H', W'}.  t = 0 gives the identity map and the page's own size.
 *
 * ocrs_unwarp_rects / ocrs_unwarp_chars (host only, in place): results found on a page warped with m, in the frame of its
 * source.  In double from the float32 coefficients.  Rects: centre X = (m0 + m1 (x + 0.5)) + m2 (y + 0.5), Y likewise;
 * up' = L up / |L up| with L = (m1 m2; m4 m5) (up stays when |L up| is 0 or not finite); w' = w * |(m1, m4)|,
 * h' = h * |(m2, m5)| (1 for a rotation); each result rounded to float32.  A rect with a value that is not finite passes
 * through as it is.  Char boxes: the four corners (points of the pixel-index frame) go through the map; left and top are
 * the floor of the minimum, right and bottom the ceil of the maximum (saturating at int32). */
typedef struct ocrs_skew_params {
    double max_deg;         /* the coarse search covers -max_deg .. +max_deg; (0, 45] */
    double coarse_step_deg; /* a whole multiple of fine_step_deg */
    double fine_step_deg;   /* > 0; the estimate's resolution */
    int32_t work_max_side;  /* 1 .. 4096 */
    int32_t reserved;       /* 0 */
} ocrs_skew_params;
typedef struct ocrs_skew_info {
    double angle_deg;       /* fine_index * fine_step_deg */
    uint64_t best_score;    /* the best coarse score */
    uint64_t second_score;  /* the runner-up among the coarse scores */
    uint64_t fine_score;    /* the score at angle_deg */
    int32_t work_h, work_w; /* the size the scores were taken at */
    int32_t coarse_index;   /* the best coarse angle, in fine steps */
    int32_t fine_index;     /* the estimate, in fine steps */
} ocrs_skew_info;
OCRS_API ocrs_status ocrs_skew_params_default(ocrs_skew_params* out);
OCRS_API ocrs_status ocrs_skew_params_check(const ocrs_skew_params* params);
OCRS_API ocrs_status ocrs_skew_table(int first, size_t n, double step_deg, int32_t* sc_table);
OCRS_API ocrs_status ocrs_engine_skew_scores(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int32_t* sc_table,
                                             size_t n_angles, uint64_t* out_scores);
OCRS_API ocrs_status ocrs_engine_estimate_skew(const ocrs_engine* e, const ocrs_page* page, const ocrs_skew_params* params,
                                               ocrs_skew_info* out);
OCRS_API ocrs_status ocrs_engine_warp_page(const ocrs_engine* e, const ocrs_page* page, int out_h, int out_w, const float m[6], float fill,
                                           ocrs_page** out);
OCRS_API ocrs_status ocrs_engine_warp_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* out_hw,
                                            const float* m, const float* fill, ocrs_page** out);
OCRS_API ocrs_status ocrs_deskew_map(int h, int w, double angle_deg, int expand, int out_hw[2], float m[6]);
OCRS_API ocrs_status ocrs_unwarp_rects(float* rects6, size_t n, const float m[6]);

/* ------------------------------------------------------------------------
 * Perspective correction (no reference counterpart, opt-in).  A sheet photographed on a desk is a keystone,
 * not a rotation: its four edges have four angles, and no affine map straightens it.  These calls find the sheet's outline
 * on a resident page without a detector, make the straightened sheet as a new resident page through a projective map, and
 * map what was found on it back to the frame of the photo.  tests/perspective_ref.py restates every definition; the library
 * equals it bit for bit.  What the outline finds on real photographs is uncalibrated: only synthetic photos exist here.
 *
 * ocrs_engine_edge_peaks: out_peaks[(((i * 2 + family) * 2 + sign) * n_angles + a) * 16 + k] for n pages of any sizes in
 * one launch (plus one small launch that takes the maxima).  sc_table as for ocrs_engine_skew_scores.  For a page of H x W
 * and min_step in 1 .. 256:
 *   q(x, y)   the bin of Page normalisation above; a NaN is not counted
 *   family 0  (H, near-horizontal lines) g(x, y) = q(x, y + 1) - q(x, y); 0 on the last row and beside a NaN.
 *             bin = (x S + y C - t0) >> 16, t0 = min(0, (W - 1) S) + min(0, (H - 1) C)
 *   family 1  (V, near-vertical lines) family 0 of the transposed page: g = q(x + 1, y) - q(x, y), bin = (y S + x C - t0T)
 *             >> 16, t0T = min(0, (H - 1) S) + min(0, (W - 1) C)
 *   sign      0 (`+`): g >= min_step; 1 (`-`): g <= -min_step.  Each such pixel adds 1 (a count, not |g|: with |g| the
 *             many strong edges of text outweigh the one long edge of the sheet) to P[family][sign][a][bin]
 *   peaks     a profile row has H + W bins, cut into 16 bands [k (H + W) / 16, (k + 1) (H + W) / 16) (integer division);
 *             per band the largest count and the smallest bin that has it, packed (count << 32) | (0xFFFFFFFF - bin); 0
 *             when the band is empty or counts nothing
 * All integers: the result does not depend on schedule, batch or launch shape.  OCRS_ERR_INVALID_ARGUMENT for n_angles < 1
 * (or > 65535), an |S| or |C| above 65536, min_step outside 1 .. 256 and a page side above 4096; OCRS_ERR_CAPACITY for more
 * than 65535 pages or more than 2 GiB of profiles (16 n_angles (H + W) bytes per page) in one call.
 *
 * ocrs_outline_choose (host only, double, no libm trigonometry): the outline among the peaks of a work_h x work_w page
 * taken from a page_h x page_w page.  At most 4095 angles, the most ocrs_engine_find_outline's own table can hold (the pair search is
 * quadratic in the peaks that count: 16 per angle, family and sign); more is OCRS_ERR_INVALID_ARGUMENT.  A peak counts when count >= ceil(min_cover L), L = work_w (family 0) or work_h
 * (family 1).  Its line is s x + c y = rho + 0.5 c (family 1: s y + c x) with s = S / 65536, c = C / 65536, rho = (bin
 * 65536 + 32768 + t0) / 65536: the edge lies between the two pixels of the difference.  Its position is its y at x =
 * (work_w - 1) / 2 (family 1: its x at y = (work_h - 1) / 2); a peak whose position is not finite is dropped.  Each sign
 * order is a hypothesis: `+` first (polarity 0) reads top and left as `+` edges, bottom and right as `-` edges: a sheet
 * lighter than the desk.  Per family the pair (first, second) of largest count1 + count2 with position2 - position1 >=
 * min_span (work_h - 1) (family 1: work_w - 1) is taken, ties to the lower (angle index, bin) of the first line, then of
 * the second; both families share the order, the order with the larger sum over the four lines wins, a tie goes to `+`
 * first.  The corners TL, TR, BR, BL are the four intersections, moved to the page's frame with (p + 0.5) (page / work) -
 * 0.5 per axis and rounded once to float32; they may lie outside the page.  found = 0 (and every other field but the work
 * size 0) when a family has no pair, a corner is not finite, the quad is not convex in this order (a consecutive cross
 * product <= 0, y down) or its area is under min_area page_h page_w.
 *
 * ocrs_engine_find_outline: (1) a page whose longer side exceeds work_max_side is shrunk with OCRS_RESAMPLE_AREA, as
 * ocrs_engine_estimate_skew does; (2) the peaks at the angles k step_deg, k = -K .. K, K = floor(max_deg / step_deg)
 * (ocrs_skew_table(-K, 2 K + 1, step_deg)); (3) ocrs_outline_choose.  params == NULL: ocrs_outline_params_default
 * (work_max_side 512, max_deg 15, step_deg 0.5, min_step 8, min_cover 0.25, min_span 0.25, min_area 0.1).
 * ocrs_outline_params_check (host only) refuses work_max_side outside 1 .. 4096, min_step outside 1 .. 256, max_deg outside
 * (0, 45], a step that is not finite and positive or that max_deg holds fewer than 1 or more than 2047 of, min_cover or
 * min_span outside (0, 1], min_area outside [0, 1].
 *
 * ocrs_quad_map (host only): corners8 = TL, TR, BR, BL as (x, y) in the page's pixel-index frame (the page's own outline
 * is (-0.5, -0.5), (W - 0.5, -0.5), (W - 0.5, H - 0.5), (-0.5, H - 0.5) and gives the identity map).  W' = floor(max(|TR -
 * TL|, |BR - BL|) + 0.5) and H' likewise from |BL - TL| and |BR - TR|, each kept within 1 .. 65535; out_hw = {H', W'}.  m =
 * Heckbert's square-to-quad coefficients with u = fx / W', v = fy / H': dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 -
 * x3 (y likewise), det = dx1 dy2 - dy1 dx2, g = (sx dy2 - sy dx2) / det, h = (dx1 sy - dy1 sx) / det; m0 = x0, m1 = (x1 -
 * x0 + g x1) / W', m2 = (x3 - x0 + h x3) / H', m3 = y0, m4 = (y1 - y0 + g y1) / W', m5 = (y3 - y0 + h y3) / H', m6 = g / W',
 * m7 = h / H'.  In double, each coefficient rounded once to float32.  OCRS_ERR_INVALID_ARGUMENT for det == 0 and for a
 * corner, a det or a coefficient that is not finite.
 *
 * ocrs_engine_project_page[s]: ocrs_engine_warp_page[s] with a projective map of eight coefficients.  float32, every
 * operation rounded on its own: fx = ox + 0.5f, fy = oy + 0.5f; nx = (m0 + m1 fx) + m2 fy, ny = (m3 + m4 fx) + m5 fy, dn =
 * (1.0f + m6 fx) + m7 fy.  When dn is finite and > 0: X = nx / dn, Y = ny / dn (correctly rounded divisions), then the taps,
 * `fill` and the lerps of ocrs_engine_warp_page; otherwise the pixel is `fill`.  With m6 = m7 = 0 the output has the bits
 * of ocrs_engine_warp_page.  Coefficients that are not finite: OCRS_ERR_INVALID_ARGUMENT.
 *
 * ocrs_unproject_rects / ocrs_unproject_chars (host only, in place): results found on a page projected with m, in the
 * frame of its source.  In double from the float32 coefficients.  Rects: the centre (x + 0.5, y + 0.5) goes through the
 * map; with J = [(m1 - m6 X) / dn, (m2 - m7 X) / dn; (m4 - m6 Y) / dn, (m5 - m7 Y) / dn], the map's Jacobian there: up' =
 * J up / |J up| (up stays when |J up| is 0 or not finite), h' = h |J up|, w' = w |J (-up.y, up.x)|; each result rounded to
 * float32.  A rect with a value that is not finite, or whose centre has dn <= 0 (or not finite), passes through as it is.
 * Char boxes: the four corners go through the map; left and top are the floor of the minimum, right and bottom the ceil of
 * the maximum (saturating at int32); a box with a corner whose dn <= 0 passes through as it is. */
typedef struct ocrs_outline_params {
    double max_deg;         /* the angles cover -max_deg .. +max_deg; (0, 45] */
    double step_deg;        /* > 0; the angles are its multiples */
    double min_cover;       /* (0, 1]: a line's edge pixels, as a share of the work page's side along it */
    double min_span;        /* (0, 1]: the distance between opposite sides, as a share of the work page's side across them */
    double min_area;        /* [0, 1]: the quad's area, as a share of the page's */
    int32_t work_max_side;  /* 1 .. 4096 */
    int32_t min_step;       /* 1 .. 256: bins between neighbouring pixels that make an edge */
} ocrs_outline_params;
typedef struct ocrs_outline_info {
    int32_t found;          /* 1: corners holds an outline */
    int32_t polarity;       /* 0: `+` first, the sheet is lighter than the desk; 1: `-` first */
    float corners[8];       /* TL, TR, BR, BL as (x, y), the page's pixel-index frame */
    uint32_t counts[4];     /* the edge pixels of top, bottom, left, right */
    int32_t angles[4];      /* their angles, as indices k + K into the table */
    int32_t work_h, work_w; /* the size the peaks were taken at */
} ocrs_outline_info;
OCRS_API ocrs_status ocrs_outline_params_default(ocrs_outline_params* out);
OCRS_API ocrs_status ocrs_outline_params_check(const ocrs_outline_params* params);
OCRS_API ocrs_status ocrs_engine_edge_peaks(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int32_t* sc_table,
                                            size_t n_angles, int min_step, uint64_t* out_peaks);
OCRS_API ocrs_status ocrs_outline_choose(const uint64_t* peaks, const int32_t* sc_table, size_t n_angles, int work_h, int work_w,
                                         int page_h, int page_w, const ocrs_outline_params* params, ocrs_outline_info* out);
OCRS_API ocrs_status ocrs_engine_find_outline(const ocrs_engine* e, const ocrs_page* page, const ocrs_outline_params* params,
                                              ocrs_outline_info* out);
OCRS_API ocrs_status ocrs_quad_map(const float corners8[8], int out_hw[2], float m[8]);
OCRS_API ocrs_status ocrs_engine_project_page(const ocrs_engine* e, const ocrs_page* page, int out_h, int out_w, const float m[8],
                                              float fill, ocrs_page** out);
OCRS_API ocrs_status ocrs_engine_project_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* out_hw,
                                               const float* m, const float* fill, ocrs_page** out);
OCRS_API ocrs_status ocrs_unproject_rects(float* rects6, size_t n, const float m[8]);

/* ------------------------------------------------------------------------
 * Ruled-line removal (no reference counterpart, opt-in).  Forms, invoices, tables, ruled paper and
 * underlined headings: a rule that touches or crosses a line of text ends up inside the word boxes and inside every
 * recognition crop cut from them.  These calls make a new resident page on which the long thin rules are overwritten with
 * the paper's level and every other pixel keeps its own 32-bit word (NaN payloads and -0.0 included); coordinates do not
 * move, so nothing needs mapping back.  The source page is untouched; release both with ocrs_page_free in any order.  The
 * page is dark ink on light paper (ocrs_engine_normalize_page makes it so) and its rules are axis-aligned (deskew first).
 * What a trained detector or recogniser gains is uncalibrated.
 *
 * The definition (tests/rules_ref.py restates it and the library equals it bit for bit; integer and set arithmetic, so the
 * result does not depend on schedule or batch).  open_h(X, n): the pixels of X in a maximal horizontal run of X of
 * length >= n; open_v the same along columns; the page edge ends a run.  With L = min_length, T = max_thickness,
 * M = margin:
 *   ink        v < threshold, an ordinary float compare: NaN is not ink, -inf is.
 *   candidates Ch = open_h(ink, L), Cv = open_v(ink, L); text = ink \ (Ch u Cv).
 *   thickness  Rh = Ch \ open_v(Ch, T + 1), Rv = Cv \ open_h(Cv, T + 1): a solid dark block is not a rule.
 *   crossings  a pixel of Rh is kept when the vertical run of Rh through it has a text pixel right above its first and
 *              right below its last pixel (a stroke that crosses the rule; a stroke that ends on it is not kept, nor is a
 *              grid intersection, text holding no candidate): Kh; Dh = Rh \ Kh.  Kv, Dv with rows and columns exchanged.
 *   margins    Mh: the pixels that are not ink within M rows of a Dh pixel of their column (the half-tone edge of an
 *              anti-aliased rule); Mv likewise along rows.  A NaN pixel is not ink and may be overwritten here.
 *   fill       the pixels that are neither ink nor NaN are counted in the bins of the normalisation above
 *              (g = clamp(v + 0.5f, 0, 1), bin = floor(g * 256f) within 0 .. 255); paper_bin = pct(1, 2), 255 with nothing
 *              counted; fill = (paper_bin + 1) / 256 - 0.5 (+0.5 on a normalised page).  With paper given (not NaN):
 *              fill = paper, paper_bin = -1, the counts are still made.
 *   output     fill on D = Dh u Dv u Mh u Mv, the page's own word elsewhere.
 *
 * ocrs_rules_params_default: threshold 0, min_length 96, max_thickness 8, margin 1, paper NaN.  ocrs_rules_params_check
 * (host only): OCRS_ERR_INVALID_ARGUMENT for a threshold that is not finite, a min_length outside 2 .. 65535, a
 * max_thickness outside 1 .. 64, a margin outside 0 .. 8 or an infinite paper; the engine calls refuse the same, and a page
 * with a side over 65535.  ocrs_engine_remove_rules_pages serves n pages of any sizes, each with its own params[i], in eight
 * launches for the whole batch on one stream; out_pages[n] receives the pages, out_infos[n] (may be NULL) what was found,
 * out_masks[n] (may be NULL) per page a host uint8 [h][w], to be released with ocrs_buffer_free: bit 0 Dh, bit 1 Dv,
 * bit 2 Mh u Mv, bit 3 Kh u Kv.  ocrs_engine_remove_rules_page: params == NULL means the default. */
typedef struct ocrs_rules_params {
    float threshold;       /* finite; ink is v < threshold */
    int32_t min_length;    /* L, 2 .. 65535 */
    int32_t max_thickness; /* T, 1 .. 64 */
    int32_t margin;        /* M, 0 .. 8 */
    float paper;           /* the fill; NaN: measured on the page */
} ocrs_rules_params;
typedef struct ocrs_rules_info {
    int32_t paper_bin;     /* the bin the fill was taken from; -1: paper was given */
    float fill;            /* what the removed pixels were overwritten with */
    uint64_t ink;          /* pixels under the threshold */
    uint64_t counted;      /* pixels that are neither ink nor NaN */
    uint64_t h_removed;    /* |Dh| */
    uint64_t v_removed;    /* |Dv| */
    uint64_t overwritten;  /* |D| */
    uint64_t kept;         /* |Kh u Kv| */
} ocrs_rules_info;
OCRS_API ocrs_status ocrs_rules_params_default(ocrs_rules_params* out);
OCRS_API ocrs_status ocrs_rules_params_check(const ocrs_rules_params* params);
OCRS_API ocrs_status ocrs_engine_remove_rules_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_rules_params* params,
                                                   ocrs_page** out_page, uint8_t** out_mask, ocrs_rules_info* out_info);
OCRS_API ocrs_status ocrs_engine_remove_rules_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                                    const ocrs_rules_params* params, ocrs_page** out_pages, uint8_t** out_masks,
                                                    ocrs_rules_info* out_infos);

/* ------------------------------------------------------------------------
 * Despeckling (no reference counterpart, opt-in).  Faxes, photocopies, dusty flatbeds and thresholded phone
 * photos carry salt-and-pepper noise: isolated dark specks on the paper become stray punctuation and spurious word boxes,
 * light pinholes inside strokes break glyphs apart.  What tells a speck from a full stop is the size of its connected
 * component, optionally with its isolation.  These calls make a new resident page on which the small ink components are
 * overwritten with the paper's level and (when asked for) the small paper components with the ink's level; every other
 * pixel keeps its own 32-bit word (NaN payloads and -0.0 included); coordinates do not move, so nothing needs mapping
 * back.  The source page is untouched; release both with ocrs_page_free in any order.  The page is dark ink on light paper
 * (ocrs_engine_normalize_page makes it so); despeckle before a deskew warp, whose interpolation smears one-pixel specks
 * into grey blobs.  What a trained detector or recogniser gains is uncalibrated.
 *
 * The definition (tests/despeckle_ref.py restates it and the library equals it bit for bit; integer and set arithmetic,
 * every set taken from the input page and nothing iterated, so the result does not depend on schedule or batch).  With
 * A = max_area, Hm = max_hole, K = keep_near:
 *   ink        v < threshold, an ordinary float compare: NaN is not ink, -inf is.
 *   components ink is 8-connected; ~ink (NaN included) is 4-connected; the page edge is a wall.
 *   candidates cand = the pixels of ink components of area <= A; big = ink \ cand.
 *   isolation  K > 0: a candidate component is kept when one of its pixels lies within Chebyshev distance K of a big pixel
 *              (i-dots, full stops and diacritics when A is large enough for real dirt); another candidate does not protect
 *              it.  speck = cand \ kept.  K = 0: nothing is kept.
 *   holes      hole = the pixels of ~ink components of area <= Hm, those at the page edge too.
 *   fills      bins as in the normalisation above (g = clamp(v + 0.5f, 0, 1), bin = floor(g * 256f) within 0 .. 255);
 *              paper_bin = pct(1, 2) of the pixels that are neither ink nor NaN, 255 with nothing counted; paper_fill =
 *              (paper_bin + 1) / 256 - 0.5.  ink_bin = pct(1, 2) of the ink pixels, 0 with no ink; ink_fill = ink_bin / 256
 *              - 0.5.  (+0.5 and -0.5 on a normalised page.)  With paper or ink_level given (not NaN) it is the fill and its
 *              bin reads -1; the counts are still made.
 *   output     paper_fill on speck, ink_fill on hole, the page's own word elsewhere.
 *
 * ocrs_speckle_params_default: threshold 0, max_area 4, max_hole 0, keep_near 0, paper NaN, ink_level NaN.  Hole filling is
 * off by default: at max_hole 2 a 512 x 512 text page lost 384 pixels of its glyphs' real counters.
 * ocrs_speckle_params_check (host only): OCRS_ERR_INVALID_ARGUMENT for a threshold that is not finite, a max_area or
 * max_hole outside 0 .. 4096, a keep_near outside 0 .. 16, an infinite paper or ink_level; the engine calls refuse the same,
 * and a page with a side over 65535 or with more than 2^31 - 1 pixels.  max_area = max_hole = 0 is valid and makes a copy.
 * ocrs_engine_despeckle_pages serves n pages of any sizes, each with its own params[i], in eight launches for the whole batch
 * on one stream; out_pages[n] receives the pages, out_infos[n] (may be NULL) what was found, out_masks[n] (may be NULL) per
 * page a host uint8 [h][w], to be released with ocrs_buffer_free: bit 0 speck, bit 1 hole, bit 2 kept.
 * ocrs_engine_despeckle_page: params == NULL means the default. */
typedef struct ocrs_speckle_params {
    float threshold;       /* finite; ink is v < threshold */
    int32_t max_area;      /* A, 0 .. 4096: the largest ink component that is a speck */
    int32_t max_hole;      /* Hm, 0 .. 4096: the largest paper component that is a pinhole */
    int32_t keep_near;     /* K, 0 .. 16: a candidate within this distance of big ink is kept; 0: none is */
    float paper;           /* the specks' fill; NaN: measured on the page */
    float ink_level;       /* the holes' fill; NaN: measured on the page */
} ocrs_speckle_params;
typedef struct ocrs_speckle_info {
    int32_t paper_bin;     /* the bin paper_fill was taken from; -1: paper was given */
    int32_t ink_bin;       /* the bin ink_fill was taken from; -1: ink_level was given */
    float paper_fill;      /* what the specks were overwritten with */
    float ink_fill;        /* what the holes were overwritten with */
    uint64_t ink;          /* pixels under the threshold */
    uint64_t counted;      /* pixels that are neither ink nor NaN */
    uint64_t specks;       /* ink components removed */
    uint64_t kept;         /* candidate components kept for being near big ink */
    uint64_t speck_pixels; /* |speck| */
    uint64_t kept_pixels;  /* |kept| */
    uint64_t holes;        /* paper components filled */
    uint64_t hole_pixels;  /* |hole| */
} ocrs_speckle_info;
OCRS_API ocrs_status ocrs_speckle_params_default(ocrs_speckle_params* out);
OCRS_API ocrs_status ocrs_speckle_params_check(const ocrs_speckle_params* params);
OCRS_API ocrs_status ocrs_engine_despeckle_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_speckle_params* params,
                                                ocrs_page** out_page, uint8_t** out_mask, ocrs_speckle_info* out_info);
OCRS_API ocrs_status ocrs_engine_despeckle_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                                 const ocrs_speckle_params* params, ocrs_page** out_pages, uint8_t** out_masks,
                                                 ocrs_speckle_info* out_infos);

/* ------------------------------------------------------------------------
 * Adaptive binarisation (no reference counterpart, opt-in).  Rule removal and despeckling above decide what
 * is ink with one threshold for the whole page; a stain, a fold shadow narrower than a normalisation tile, show-through or
 * faint ink beside dark ink defeat any single cut.  These calls make a new resident page of the same size on which every
 * pixel that Sauvola's local rule calls ink is written at the ink level and every other counted pixel at the paper level;
 * a NaN pixel keeps its own 32-bit word (payload included); coordinates do not move, so nothing needs mapping back.  The
 * source page is untouched; release both with ocrs_page_free in any order.  The page is dark ink on light paper
 * (ocrs_engine_normalize_page makes it so).  On the result ocrs_engine_remove_rules_page and ocrs_engine_despeckle_page at
 * threshold 0 use the local decision.  What a trained detector or recogniser gains is uncalibrated.
 *
 * The definition (tests/binarize_ref.py restates it and the library equals it bit for bit; integers only, every sum a plain
 * sum, so the result does not depend on schedule or batch).  With r = radius, kq = k_q8 and R = 128:
 *   bins       as in the normalisation above: g = clamp(v + 0.5f, 0, 1), b = floor(g * 256f) within 0 .. 255 (so +inf is
 *              bin 255 and -inf bin 0); NaN is not counted.
 *   window     of pixel (y, x): [y - r, y + r] x [x - r, x + r] clipped to the page; the page edge is a wall, nothing is
 *              mirrored or padded.  Over its counted pixels n is their number, S the sum of their bins, Q the sum of the
 *              squares of their bins.  A counted pixel is in its own window: n >= 1.
 *   decision   Sauvola: T = m (1 + k (s / R - 1)), m = S / n, s = sqrt(Q / n - m^2), k = kq / 256; ink is b < T.
 *              Multiplied out: V = n Q - S^2, A = n R (256 (b n - S) + kq S), B = kq S;
 *              ink <=> A < B sqrt(V) <=> A < 0 or A^2 < B^2 V, compared exactly (128 bits).  The strict < decides ties: a
 *              flat window (V = 0) has no ink, so a blank page comes back as paper and so does an all-black one (Sauvola's
 *              known behaviour).  kq = 0 is the plain local mean: b n < S.
 *   output     keep_ink = 0: ink_level on ink, paper on every other counted pixel.  keep_ink = 1: the page's own 32-bit word
 *              on ink (no arithmetic: -0.0 and out-of-range values survive), paper elsewhere: background whitening that
 *              leaves the grey edges of the strokes to the recogniser.  NaN pixels keep their word in both modes.
 *
 * ocrs_binarize_params_default: radius 15, k_q8 87 (k = 0.34), keep_ink 0, ink_level NaN (-0.5f), paper NaN (+0.5f).
 * ocrs_binarize_params_check (host only): OCRS_ERR_INVALID_ARGUMENT for a radius outside 1 .. 127, a k_q8 outside 0 .. 256, a
 * keep_ink that is neither 0 nor 1, an infinite ink_level or paper; the engine calls refuse the same, and a page with a
 * side over 65535 or with more than 2^31 - 1 pixels.
 * ocrs_engine_binarize_pages serves n pages of any sizes, each with its own params[i], in three launches for the whole
 * batch on one stream; out_pages[n] receives the pages, out_infos[n] (may be NULL) the counts and the fills used,
 * out_masks[n] (may be NULL) per page a host uint8 [h][w], to be released with ocrs_buffer_free: bit 0 ink.
 * ocrs_engine_binarize_page: params == NULL means the default. */
typedef struct ocrs_binarize_params {
    int32_t radius;        /* r, 1 .. 127: the window is (2 r + 1) x (2 r + 1) */
    int32_t k_q8;          /* kq, 0 .. 256: Sauvola's k in 1/256 */
    int32_t keep_ink;      /* 0: ink is written at ink_level; 1: ink keeps its own word */
    float ink_level;       /* the fill of ink; NaN: -0.5f; not infinite */
    float paper;           /* the fill of every other counted pixel; NaN: +0.5f; not infinite */
} ocrs_binarize_params;
typedef struct ocrs_binarize_info {
    uint64_t counted;      /* pixels that are not NaN */
    uint64_t ink;          /* counted pixels the local rule calls ink */
    float ink_fill;        /* the ink fill used (with keep_ink it is not written) */
    float paper_fill;      /* the paper fill used */
} ocrs_binarize_info;
OCRS_API ocrs_status ocrs_binarize_params_default(ocrs_binarize_params* out);
OCRS_API ocrs_status ocrs_binarize_params_check(const ocrs_binarize_params* params);
OCRS_API ocrs_status ocrs_engine_binarize_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_binarize_params* params,
                                               ocrs_page** out_page, uint8_t** out_mask, ocrs_binarize_info* out_info);
OCRS_API ocrs_status ocrs_engine_binarize_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                                const ocrs_binarize_params* params, ocrs_page** out_pages, uint8_t** out_masks,
                                                ocrs_binarize_info* out_infos);

/* ------------------------------------------------------------------------
 * Stroke repair (no reference counterpart, opt-in).  Everything above leaves the shape of the ink as it
 * is; faint faxes, dot-matrix and thermal printouts, worn ribbons and copies of copies have strokes broken into pieces,
 * over-inked prints have them fused.  These calls make a new resident page of the same size by grey-level morphology:
 * running minima and maxima over a rectangle around every pixel.  A result pixel is always the 32-bit word of some pixel
 * of the source, never a recomputed number; a NaN pixel keeps its own word (payload included); coordinates do not move, so
 * nothing needs mapping back.  The source page is untouched; release both with ocrs_page_free in any order.  The page is
 * dark ink on light paper (ocrs_engine_normalize_page makes it so).  What a trained detector or recogniser gains is
 * uncalibrated.
 *
 * The definition (tests/morph_ref.py restates it and the library equals it bit for bit; nothing is computed, so the result
 * does not depend on schedule or batch):
 *   order      pixels are ordered as 32-bit words w through the key k(w) = ~w if the sign bit is set, else w | 0x80000000:
 *              -inf < ... < -0.0 < +0.0 < ... < +inf, denormals in their places, -0.0 and +0.0 two values.  NaN of any
 *              payload is not counted: it enters no window.
 *   window     of pixel (y, x): [y - ry, y + ry] x [x - rx, x + rx] clipped to the page; the page edge is a wall, nothing
 *              is mirrored or padded.  A counted pixel is in its own window.
 *   stages     lo: every counted pixel becomes the word of least key among the counted pixels of its window; hi: of the
 *              greatest key.  A second stage reads the first stage's page under the same rules.
 *   ops        named for what happens to the ink (dark): OCRS_MORPH_THICKEN = lo (ink grows), OCRS_MORPH_THIN = hi (ink
 *              shrinks), OCRS_MORPH_CLOSE = lo then hi (gaps and breaks in the ink narrower than the window are bridged,
 *              everything else keeps its extent), OCRS_MORPH_OPEN = hi then lo (hairs and bridges of ink narrower than the
 *              window vanish; fused characters separate).
 *
 * ocrs_morph_params_default: close, rx 1, ry 1.
 * ocrs_morph_params_check (host only): OCRS_ERR_INVALID_ARGUMENT for an op outside 0 .. 3, an rx or ry outside 0 .. 63, or
 * both 0; the engine calls refuse the same, and a page with a side over 65535 or with more than 2^31 - 1 pixels.
 * ocrs_engine_morph_pages serves n pages of any sizes, each with its own params[i] (ops and radii mix freely), in at most
 * five launches for the whole batch on one stream; out_pages[n] receives the pages, out_infos[n] (may be NULL) the counts,
 * out_masks[n] (may be NULL) per page a host uint8 [h][w], to be released with ocrs_buffer_free: bit 0 ink after (counted
 * and under 0.0f), bit 1 the word changed.
 * ocrs_engine_morph_page: params == NULL means the default. */
#define OCRS_MORPH_THICKEN 0
#define OCRS_MORPH_THIN 1
#define OCRS_MORPH_CLOSE 2
#define OCRS_MORPH_OPEN 3
typedef struct ocrs_morph_params {
    int32_t op;            /* OCRS_MORPH_* */
    int32_t rx;            /* 0 .. 63: the window is (2 ry + 1) rows of (2 rx + 1) pixels */
    int32_t ry;            /* 0 .. 63; not both 0 */
} ocrs_morph_params;
typedef struct ocrs_morph_info {
    uint64_t counted;      /* pixels that are not NaN */
    uint64_t changed;      /* counted pixels whose word changed */
    uint64_t ink_before;   /* counted pixels under 0.0f on the source */
    uint64_t ink_after;    /* counted pixels under 0.0f on the result */
} ocrs_morph_info;
OCRS_API ocrs_status ocrs_morph_params_default(ocrs_morph_params* out);
OCRS_API ocrs_status ocrs_morph_params_check(const ocrs_morph_params* params);
OCRS_API ocrs_status ocrs_engine_morph_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_morph_params* params,
                                            ocrs_page** out_page, uint8_t** out_mask, ocrs_morph_info* out_info);
OCRS_API ocrs_status ocrs_engine_morph_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                             const ocrs_morph_params* params, ocrs_page** out_pages, uint8_t** out_masks,
                                             ocrs_morph_info* out_infos);

/* ------------------------------------------------------------------------
 * Grain removal (no reference counterpart, opt-in).  Sensor noise of a photo taken in poor light, salt and
 * pepper on a grey page, a halftone screen under the text: despeckling sees them only after a threshold has turned them
 * into components and cannot touch salt inside strokes, stroke repair removes one polarity by growing the other, and
 * binarisation turns grain into specks.  These calls make a new resident page of the same size by a rank filter over a
 * rectangle around every pixel: a median, any percentile, or either applied to outliers only, so that hairlines and small
 * print survive.  It belongs in front of the threshold.  A result pixel is always the 32-bit word of some pixel of the
 * source, never a recomputed number; a NaN pixel keeps its own word (payload included); coordinates do not move, so nothing
 * needs mapping back.  The source page is untouched; release both with ocrs_page_free in any order.  What a trained
 * detector or recogniser gains is uncalibrated.
 *
 * The definition (tests/rank_ref.py restates it and the library equals it bit for bit; nothing is computed, so the result
 * does not depend on schedule or batch):
 *   order      stroke repair's: words w are ordered through the key k(w) = ~w if the sign bit is set, else w | 0x80000000;
 *              -0.0 and +0.0 are two values.  NaN of any payload is not counted: it enters no window.
 *   window     of pixel (y, x): [y - ry, y + ry] x [x - rx, x + rx] clipped to the page; at most 15 x 15.  A counted pixel
 *              is in its own window, so the number n of counted pixels in it is at least 1.
 *   rank       at(p) = (p (n - 1) + 50) / 100 in integers; s[0 .. n - 1] the window's counted keys in ascending order.  The
 *              filter's value is the word of s[at(percent)]: percent 0 the least key (stroke repair's thicken), 100 the
 *              greatest (thin), 50 the median, of an even n the upper one.
 *   sparing    tail = 0: every counted pixel takes the filter's value.  tail >= 1: with lt the number of window keys under
 *              the pixel's own key and le the number under or equal, the pixel keeps its word iff lt <= at(100 - tail) and
 *              le - 1 >= at(tail): its own ranks meet the central part of its window, it is no outlier.  percent 50 with
 *              tail 50 is percent 50 with tail 0; a tail so small that at(tail) = 0 spares every pixel.
 *
 * ocrs_rank_params_default: rx 1, ry 1, percent 50, tail 20.
 * ocrs_rank_params_check (host only): OCRS_ERR_INVALID_ARGUMENT for an rx or ry outside 0 .. 7 or both 0, a percent outside
 * 0 .. 100, a tail outside 0 .. 50; the engine calls refuse the same, and a page with a side over 65535 or with more than
 * 2^31 - 1 pixels.
 * ocrs_engine_rank_pages serves n pages of any sizes, each with its own params[i] (radii, percents and tails mix freely), in
 * at most three launches for the whole batch on one stream; out_pages[n] receives the pages, out_infos[n] (may be NULL) the counts,
 * out_masks[n] (may be NULL) per page a host uint8 [h][w], to be released with ocrs_buffer_free: bit 0 ink after (counted
 * and under 0.0f), bit 1 the word changed.  A failed call writes no output pointer and leaves nothing allocated.
 * ocrs_engine_rank_page: params == NULL means the default. */
typedef struct ocrs_rank_params {
    int32_t rx;            /* 0 .. 7: the window is (2 ry + 1) rows of (2 rx + 1) pixels */
    int32_t ry;            /* 0 .. 7; not both 0 */
    int32_t percent;       /* 0 .. 100: the rank taken, 50 the median */
    int32_t tail;          /* 0 .. 50: a pixel whose ranks lie inside [tail, 100 - tail] percent keeps its word; 0: none does */
} ocrs_rank_params;
typedef struct ocrs_rank_info {
    uint64_t counted;      /* pixels that are not NaN */
    uint64_t changed;      /* counted pixels whose word changed */
    uint64_t ink_before;   /* counted pixels under 0.0f on the source */
    uint64_t ink_after;    /* counted pixels under 0.0f on the result */
    uint64_t spared;       /* counted pixels that kept their word by the sparing rule */
} ocrs_rank_info;
OCRS_API ocrs_status ocrs_rank_params_default(ocrs_rank_params* out);
OCRS_API ocrs_status ocrs_rank_params_check(const ocrs_rank_params* params);
OCRS_API ocrs_status ocrs_engine_rank_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_rank_params* params,
                                           ocrs_page** out_page, uint8_t** out_mask, ocrs_rank_info* out_info);
OCRS_API ocrs_status ocrs_engine_rank_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                            const ocrs_rank_params* params, ocrs_page** out_pages, uint8_t** out_masks,
                                            ocrs_rank_info* out_infos);

/* ------------------------------------------------------------------------
 * Page framing (no reference counterpart, opt-in).  What surrounds the text: the black bars of photocopies
 * and flatbed scans, the dark wedge a skewed sheet leaves, the slice of the neighbouring page and the gutter shadow of a
 * book scan, the two pages of a spread.  The detector turns such bars into word boxes and the line finder joins the two
 * pages of a spread; despeckling refuses anything over 4096 pixels and rule removal anything thicker than max_thickness.
 * Four pieces, each usable alone: frame cleanup, ink profiles, the choice of the content box and the gutter, and the crop
 * with its maps back.  The page is dark ink on light paper (ocrs_engine_normalize_page makes it so; bars survive a
 * binarisation).  What a trained detector or recogniser gains is uncalibrated.
 *
 * 1. Frame cleanup makes a new resident page of the same size on which the ink that is connected to the page frame is
 * overwritten with the paper's level; every other pixel keeps its own 32-bit word (NaN payloads and -0.0 included);
 * coordinates do not move.  The definition (tests/frame_ref.py restates it and the library equals it bit for bit; integer
 * and set arithmetic, nothing iterated, so the result does not depend on schedule or batch).  With D = depth:
 *   ink        v < threshold, an ordinary float compare: NaN is not ink, -inf is.
 *   ring       d(y, x) = min(x, y, w - 1 - x, h - 1 - y); D = 0: the whole page; D > 0: the pixels with d < D.  Nothing
 *              deeper than D is ever changed: the bound on the damage when a table frame or an underline runs off the sheet.
 *   components R = ink in the ring, 8-connected; the page edge and the ring's inner edge are walls: a stroke that leaves
 *              the ring and comes back in is two components.
 *   seeds      the pixels of R on an enabled side; `sides` bit 0 left (x = 0), 1 top (y = 0), 2 right (x = w - 1), 3 bottom
 *              (y = h - 1).
 *   classes    a component holding a seed is touching; its area is its number of pixels in R.  removed = the pixels of
 *              touching components of area >= min_area; kept = those of touching components of area < min_area (a glyph cut
 *              by the edge of a tight screenshot crop).
 *   fill       despeckling's paper fill: paper_bin = pct(1, 2) of the pixels of the whole page that are neither ink nor
 *              NaN, 255 with nothing counted; paper_fill = (paper_bin + 1) / 256 - 0.5.  With paper given (not NaN) it is
 *              the fill and the bin reads -1.
 *   output     paper_fill on removed, the page's own word elsewhere.
 * ocrs_frame_params_default: threshold 0, depth 128, sides 15, min_area 0, paper NaN.  ocrs_frame_params_check (host only):
 * OCRS_ERR_INVALID_ARGUMENT for a threshold that is not finite, a depth outside 0 .. 65535, sides outside 1 .. 15, a negative
 * min_area, an infinite paper; the engine calls refuse the same, and a page with a side over 65535 or with more than
 * 2^31 - 1 pixels.  ocrs_engine_clean_frame_pages serves n pages of any sizes, each with its own params[i], in six launches
 * for the whole batch on one stream; out_pages[n] receives the pages, out_infos[n] (may be NULL) what was found,
 * out_masks[n] (may be NULL) per page a host uint8 [h][w], to be released with ocrs_buffer_free: bit 0 removed, bit 1 kept,
 * bit 2 in R.  ocrs_engine_clean_frame_page: params == NULL means the default.
 *
 * 2. ocrs_engine_ink_profiles counts the pixels with v < threshold (finite) per column into out_cols[w] and per row into
 * out_rows[h]; either may be NULL.  One launch; integer sums, exact whatever the order.
 *
 * 3. ocrs_frame_choose (host only) makes the content box and the gutter of a spread out of the two profiles:
 *   content    cx0 = the first column with col_ink >= min_count, cx1 = the last such column + 1; rows likewise.  None:
 *              found = 0 and the box is the whole page.  Otherwise the box is [cx0 - pad, cx1 + pad) x [cy0 - pad, cy1 + pad)
 *              clipped to the page.
 *   gutter     only when found, otherwise -1.  band = [cx0 + 3 (cx1 - cx0) / 8, cx0 + 5 (cx1 - cx0) / 8), floor division.  A
 *              column is quiet when col_ink <= gutter_max_ink.  Among the maximal runs of quiet columns inside the band the
 *              longest; ties to the least |2 mid - (cx0 + cx1)| with mid = start + len / 2, then to the leftmost.  Its
 *              length >= gutter_min_width: gutter_x = mid, otherwise -1.  The left page is [x0, gutter_x), the right page
 *              [gutter_x, x1).
 * ocrs_frame_choice_params_default: min_count 1, pad 16, gutter_min_width 8, gutter_max_ink 0; _check: INVALID_ARGUMENT for
 * min_count < 1, pad outside 0 .. 65535, gutter_min_width < 1, gutter_max_ink < 0.  ocrs_frame_choose refuses the same and
 * sides outside 1 .. 65535; params == NULL means the default.
 *
 * 4. ocrs_engine_crop_pages cuts rects[i] = [x0, x1) x [y0, y1) out of pages[i] as a new resident page of (y1 - y0) x
 * (x1 - x0), each side 1 .. 65535 (otherwise INVALID_ARGUMENT), for pages of any mix of sizes in one launch.  The rectangle
 * may lie partly or wholly outside the page: an outside pixel is the 32-bit word of fill[i], whatever its bits, an inside
 * pixel the source's word; a crop that adds margins is a valid use.  ocrs_uncrop_rects / ocrs_uncrop_chars (declared with
 * ocrs_unrotate_rects below; host only, in place): results found on the cropped page mapped back to the frame of the page
 * it was cut from: the centre of a rect gets one float32 addition of the offset per coordinate, char boxes get integer
 * addition, everything else is untouched. */
typedef struct ocrs_frame_params {
    float threshold;       /* finite; ink is v < threshold */
    int32_t depth;         /* D, 0 .. 65535: the ring's depth; 0: the whole page */
    int32_t sides;         /* 1 .. 15: bit 0 left, 1 top, 2 right, 3 bottom */
    int32_t min_area;      /* >= 0: a touching component smaller than this is kept */
    float paper;           /* the fill; NaN: measured on the page */
} ocrs_frame_params;
typedef struct ocrs_frame_info {
    int32_t paper_bin;     /* the bin paper_fill was taken from; -1: paper was given */
    float paper_fill;      /* what the removed ink was overwritten with */
    uint64_t ink;          /* pixels under the threshold */
    uint64_t counted;      /* pixels that are neither ink nor NaN */
    uint64_t ring_ink;     /* |R| */
    uint64_t removed;      /* touching components removed */
    uint64_t removed_pixels; /* |removed| */
    uint64_t kept;         /* touching components kept for being smaller than min_area */
    uint64_t kept_pixels;  /* |kept| */
} ocrs_frame_info;
typedef struct ocrs_frame_choice_params {
    int32_t min_count;         /* >= 1 */
    int32_t pad;               /* 0 .. 65535 */
    int32_t gutter_min_width;  /* >= 1 */
    int32_t gutter_max_ink;    /* >= 0 */
} ocrs_frame_choice_params;
typedef struct ocrs_frame_choice {
    int32_t found;             /* 1: there is content */
    int32_t x0, y0, x1, y1;    /* the box, half open */
    int32_t gutter_x;          /* the right page's first column; -1: no gutter */
} ocrs_frame_choice;
typedef struct ocrs_crop_rect {
    int32_t x0, y0, x1, y1;    /* half open; may reach outside the page */
} ocrs_crop_rect;
OCRS_API ocrs_status ocrs_frame_params_default(ocrs_frame_params* out);
OCRS_API ocrs_status ocrs_frame_params_check(const ocrs_frame_params* params);
OCRS_API ocrs_status ocrs_engine_clean_frame_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_frame_params* params,
                                                  ocrs_page** out_page, uint8_t** out_mask, ocrs_frame_info* out_info);
OCRS_API ocrs_status ocrs_engine_clean_frame_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                                   const ocrs_frame_params* params, ocrs_page** out_pages, uint8_t** out_masks,
                                                   ocrs_frame_info* out_infos);
OCRS_API ocrs_status ocrs_engine_ink_profiles(const ocrs_engine* e, const ocrs_page* page, float threshold, uint32_t* out_cols,
                                              uint32_t* out_rows);
OCRS_API ocrs_status ocrs_frame_choice_params_default(ocrs_frame_choice_params* out);
OCRS_API ocrs_status ocrs_frame_choice_params_check(const ocrs_frame_choice_params* params);
OCRS_API ocrs_status ocrs_frame_choose(int h, int w, const uint32_t* col_ink, const uint32_t* row_ink,
                                       const ocrs_frame_choice_params* params, ocrs_frame_choice* out);
OCRS_API ocrs_status ocrs_engine_crop_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_crop_rect* rect, float fill,
                                           ocrs_page** out_page);
OCRS_API ocrs_status ocrs_engine_crop_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_crop_rect* rects,
                                            const float* fill, ocrs_page** out_pages);

/* ------------------------------------------------------------------------
 * Page measurement (no reference counterpart, opt-in).  Every parameter of the page operations above is in
 * pixels, and a good value depends on how large the text of this scan is.  This measures it on the device, without a
 * detector: the page's stroke width from run-length histograms and its text height from the bounding boxes of its connected
 * components, so that the working resolution ("Working resolution" above) can follow from the page instead of being set
 * blind.  No page is made and no pixel is written.  The page is dark ink on light paper (ocrs_engine_normalize_page makes it
 * so).  What a trained detector gains from the derived scale is uncalibrated.
 *
 * 1. ocrs_engine_measure_pages fills out_infos[n] for n pages of any sizes, each with its own params[i], in five launches
 * for the whole batch on one stream.  The definition (tests/measure_ref.py restates it and the library equals it in every
 * field and bin; integer and set arithmetic, so the record does not depend on schedule or batch):
 *   ink        v < threshold, an ordinary float compare: NaN is not ink, v == threshold is not, -inf is.
 *   components the 8-connected components of ink; the page edge is a wall.  counted: those of area >= min_area.
 *   run_h, run_v  the maximal horizontal / vertical runs of ink by their length L, at index min(L, 255); the page edge ends a
 *              run; index 0 stays 0.
 *   comp_h, comp_w  the counted components by the height / width of their bounding box, at index min(side, 255).
 *   area_by_h  the summed areas of the counted components, by the index of comp_h.
 * ocrs_measure_params_default: threshold 0, min_area 4.  ocrs_measure_params_check (host only): OCRS_ERR_INVALID_ARGUMENT for
 * a threshold that is not finite or a min_area outside 0 .. 65535; the engine calls refuse the same, and a page with a side
 * over 65535 or with more than 2^31 - 1 pixels.  The workspace is 20 bytes and one bit per pixel; a batch of more than 2^31
 * tiles of 64 x 64, or whose workspace exceeds the device's memory, fails with OCRS_ERR_CAPACITY before anything is launched.
 * n == 0 succeeds and launches nothing.  A call that fails writes no output.  ocrs_engine_measure_page: params == NULL means
 * the default.
 *
 * 2. ocrs_measure_choose (host only) makes a scale out of one record:
 *   stroke     with r[L] = run_h[L] + run_v[L], the L in 1 .. 254 that maximises L * r[L], the pixels that lie in runs of that
 *              length; the smallest L on a tie; 0 when no run is shorter than 255.
 *   text_height  min_height_strokes is taken in 1/256: q = floor(min_height_strokes * 256 + 0.5).  A height H in 1 .. 254
 *              qualifies when 256 H >= q * stroke (integers).  support = the counted components of a qualifying height.
 *              text_height = the lower median of the qualifying heights by ink: the smallest qualifying H at which the
 *              cumulative area_by_h reaches half of its sum over the qualifying heights, rounded up; 0 with no support.
 *              Bin 255 (a picture, a rule) never qualifies; dots, commas and dashes hold next to no ink.
 *   blank      support == 0.
 * ocrs_measure_choice_params_default: min_height_strokes 0.5; _check: INVALID_ARGUMENT unless it is finite and 0 .. 255.
 * ocrs_measure_choose refuses the same; params == NULL means the default.
 *
 * 3. ocrs_work_scale_for_text (host only): *scale = target_height / text_height clamped to [min_scale, max_scale], in double;
 * 1.0 for text_height <= 0 (a blank page keeps its size).  INVALID_ARGUMENT unless target_height is finite and positive and
 * 0 < min_scale <= max_scale, both finite.  Its result feeds ocrs_work_size.  OCRS_WORK_TEXT_HEIGHT_DEFAULT is the text
 * height tests/measure_ref.py finds on the benchmark's synthetic pages, the size the synthetic detector
 * was made for; for real models it is uncalibrated. */
#define OCRS_MEASURE_BINS 256
#define OCRS_WORK_TEXT_HEIGHT_DEFAULT 14
typedef struct ocrs_measure_params {
    float threshold;       /* finite; ink is v < threshold */
    int32_t min_area;      /* 0 .. 65535: a component of fewer pixels is a speck and is not counted */
} ocrs_measure_params;
typedef struct ocrs_measure_info {
    uint64_t ink;          /* pixels under the threshold */
    uint32_t components;   /* 8-connected components of ink */
    uint32_t counted;      /* those of area >= min_area */
    uint32_t run_h[OCRS_MEASURE_BINS];      /* horizontal runs by min(length, 255) */
    uint32_t run_v[OCRS_MEASURE_BINS];      /* vertical runs by min(length, 255) */
    uint32_t comp_h[OCRS_MEASURE_BINS];     /* counted components by min(box height, 255) */
    uint32_t comp_w[OCRS_MEASURE_BINS];     /* counted components by min(box width, 255) */
    uint64_t area_by_h[OCRS_MEASURE_BINS];  /* their summed areas by min(box height, 255) */
} ocrs_measure_info;
typedef struct ocrs_measure_choice_params {
    double min_height_strokes;  /* 0 .. 255, taken in 1/256 */
} ocrs_measure_choice_params;
typedef struct ocrs_text_scale {
    int32_t stroke;        /* pixels; 0: no run shorter than 255 */
    int32_t text_height;   /* pixels; 0: blank */
    uint32_t support;      /* the components that entered the median */
    int32_t blank;         /* 1: support == 0 */
} ocrs_text_scale;
OCRS_API ocrs_status ocrs_measure_params_default(ocrs_measure_params* out);
OCRS_API ocrs_status ocrs_measure_params_check(const ocrs_measure_params* params);
OCRS_API ocrs_status ocrs_engine_measure_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_measure_params* params,
                                              ocrs_measure_info* out_info);
OCRS_API ocrs_status ocrs_engine_measure_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                               const ocrs_measure_params* params, ocrs_measure_info* out_infos);
OCRS_API ocrs_status ocrs_measure_choice_params_default(ocrs_measure_choice_params* out);
OCRS_API ocrs_status ocrs_measure_choice_params_check(const ocrs_measure_choice_params* params);
OCRS_API ocrs_status ocrs_measure_choose(const ocrs_measure_info* info, const ocrs_measure_choice_params* params, ocrs_text_scale* out);
OCRS_API ocrs_status ocrs_work_scale_for_text(int text_height, double target_height, double min_scale, double max_scale, double* scale);

/* ------------------------------------------------------------------------
 * Reverse-video repair (no reference counterpart, opt-in).  Every page operation above takes one polarity
 * for the whole page, but a table's header row in white on a dark band, the buttons, banners and sidebars of a screenshot, a
 * dark code pane beside a light document, a pull-quote or the reversed title block of a form are light text on a solid dark
 * panel.  There the panel is "ink" and its text "paper": a whole-page inversion only swaps which half of the page is lost.
 * These calls make a new resident page of the same size on which the solid dark panels that enclose light marks, and what
 * they enclose, are inverted: pages are centred on 0, so the sign bit of those pixels is flipped.  Every result pixel is the
 * source's 32-bit word or that word XOR 0x80000000 (NaN payloads, -0.0 and denormals included); coordinates do not move,
 * so nothing needs mapping back.  The source page is untouched; release both with ocrs_page_free in any order.  Call it
 * before ocrs_engine_clean_frame_page, which would remove a sidebar that touches the edge as a bar.  What a trained
 * detector or recogniser gains is uncalibrated.
 *
 * The definition (tests/reverse_ref.py restates it and the library equals it bit for bit; integer and set arithmetic on
 * sets taken from the input page, nothing iterated but the labelling, so the result does not depend on schedule or batch):
 *   ink        v < threshold, an ordinary float compare: NaN is not ink, v == threshold is not.  Its 8-connected components
 *              have an area A and a bounding box of bh x bw; the page edge is a wall.
 *   candidates a component with bh >= min_height, bw >= min_width and 256 A >= q bh bw in 64-bit integers, q = floor(256
 *              min_fill + 0.5) in float.  M = the candidates' pixels.  A table grid or a page frame fails the fill test, a
 *              letter the size test.
 *   holes      everything outside M (paper, NaN, the ink of non-candidates) is 4-connected.  A component that holds a pixel
 *              of the page's first or last row or column is open; every other is a hole of area a.  Its encloser is the
 *              candidate that owns the pixel west of the hole's raster-first pixel (least row, then least column).  A hole
 *              counts when max_hole == 0 or a <= max_hole: a large light card inside a panel stays as it is.
 *   panels     a candidate that is the encloser of at least min_holes counting holes.  The default of 3 keeps a bold
 *              headline O, B or 8 out; with 0 every candidate is a panel and solid bars turn white.
 *   output     the sign bit flipped on every pixel of a panel and of a counting hole whose encloser is a panel; the page's
 *              own word elsewhere.
 * Not covered: a panel whose light text touches the panel's edge (open, not a hole), light text on dark with no solid
 * panel around it, nested panels beyond what the definition gives.
 *
 * ocrs_reverse_params_default: threshold 0, min_height 32, min_width 64, min_fill 0.4, min_holes 3, max_hole 0.  All five
 * are UNCALIBRATED: no real scans stand behind them.
 * ocrs_reverse_params_check (host only): OCRS_ERR_INVALID_ARGUMENT for a threshold that is not finite, a min_height or
 * min_width outside 1 .. 65535, a min_fill outside [0, 1] or NaN, a negative min_holes or max_hole; the engine calls refuse
 * the same, and a page with a side over 65535 or with more than 2^31 - 1 pixels; OCRS_ERR_CAPACITY for a batch of more than
 * 2^31 tiles of 64 x 64 or whose workspace (20 bytes a pixel) exceeds the device's memory, before anything is allocated.
 * ocrs_engine_unreverse_pages serves n pages of any sizes, each with its own params[i], in nine launches for the whole batch
 * on one stream; out_pages[n] receives the pages, out_infos[n] (may be NULL) what was found, out_masks[n] (may be NULL) per
 * page a host uint8 [h][w], to be released with ocrs_buffer_free: bit 0 inverted, bit 1 in M, bit 2 in a panel, bit 3 in a
 * hole (counting or not, whatever its encloser).
 * ocrs_engine_unreverse_page: params == NULL means the default. */
typedef struct ocrs_reverse_params {
    float threshold;       /* finite; ink is v < threshold */
    int32_t min_height;    /* 1 .. 65535: the least height of a candidate's box (default 32, uncalibrated) */
    int32_t min_width;     /* 1 .. 65535: the least width of a candidate's box (default 64, uncalibrated) */
    float min_fill;        /* [0, 1]: the least share of its box a candidate fills, taken in 1/256 (default 0.4, uncalibrated) */
    int32_t min_holes;     /* >= 0: the counting holes that make a candidate a panel (default 3, uncalibrated) */
    int32_t max_hole;      /* >= 0 pixels: the largest hole that counts and is inverted; 0: no limit (default 0, uncalibrated) */
} ocrs_reverse_params;
typedef struct ocrs_reverse_info {
    uint64_t ink;            /* pixels under the threshold */
    uint64_t components;     /* 8-connected components of ink */
    uint64_t candidates;     /* those large and solid enough */
    uint64_t panels;         /* candidates with at least min_holes counting holes */
    uint64_t panel_pixels;   /* their pixels */
    uint64_t holes;          /* counting holes of panels */
    uint64_t hole_pixels;    /* their pixels */
    uint64_t skipped_holes;  /* holes of panels over max_hole: not inverted */
    uint64_t inverted;       /* panel_pixels + hole_pixels */
} ocrs_reverse_info;
OCRS_API ocrs_status ocrs_reverse_params_default(ocrs_reverse_params* out);
OCRS_API ocrs_status ocrs_reverse_params_check(const ocrs_reverse_params* params);
OCRS_API ocrs_status ocrs_engine_unreverse_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_reverse_params* params,
                                                ocrs_page** out_page, uint8_t** out_mask, ocrs_reverse_info* out_info);
OCRS_API ocrs_status ocrs_engine_unreverse_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n,
                                                 const ocrs_reverse_params* params, ocrs_page** out_pages, uint8_t** out_masks,
                                                 ocrs_reverse_info* out_infos);

/* OcrEngine::detection_threshold (lib.rs:282-287). */
OCRS_API float ocrs_engine_detection_threshold(const ocrs_engine* e);

/* OcrEngine::find_text_lines (lib.rs:222-228 -> layout_analysis.rs:158-233).
 * Host-side.  *line_rects receives the same n_words rects permuted into
 * reading order; line i owns rects [line_offsets[i], line_offsets[i+1]). */
OCRS_API ocrs_status ocrs_engine_find_text_lines(const ocrs_engine* e, const ocrs_page* page, const float* word_rects,
                                        size_t n_words, float** line_rects, size_t** line_offsets,
                                        size_t* n_lines);

/* The same for several pages at once (one host thread per page).  Words of page p
 * are word_rects[6*word_offsets[p] .. 6*word_offsets[p+1]).  *line_rects receives all
 * words, permuted into reading order page by page; line i (numbered across pages) owns
 * rects [line_offsets[i], line_offsets[i+1]); page p owns lines
 * [page_line_offsets[p], page_line_offsets[p+1]). */
OCRS_API ocrs_status ocrs_engine_find_text_lines_batch(const ocrs_engine* e, size_t n_pages, const float* word_rects,
                                                       const size_t* word_offsets, float** line_rects,
                                                       size_t** line_offsets, size_t** page_line_offsets);

/* The two calls above, plus *word_index (malloc'ed, one entry per output rect): word_index[k] is the index, within its
 * page's input words, of output rect k — what a caller needs to carry anything per word (a detection score, a label)
 * across the permutation.  A permutation per page; identical input rects keep distinct indices. */
OCRS_API ocrs_status ocrs_engine_find_text_lines_indexed(const ocrs_engine* e, const ocrs_page* page, const float* word_rects,
                                                         size_t n_words, float** line_rects, size_t** line_offsets,
                                                         size_t* n_lines, size_t** word_index);
OCRS_API ocrs_status ocrs_engine_find_text_lines_batch_indexed(const ocrs_engine* e, size_t n_pages, const float* word_rects,
                                                               const size_t* word_offsets, float** line_rects,
                                                               size_t** line_offsets, size_t** page_line_offsets,
                                                               size_t** word_index);

/* One recognised character: TextChar (text_items.rs:48-54). */
typedef struct ocrs_text_char {
    uint32_t ch;                      /* Unicode scalar value */
    int32_t top, left, bottom, right; /* rten_imageproc::Rect */
} ocrs_text_char;

/* OcrEngine::recognize_text (lib.rs:237-256 -> recognition.rs:404-540).
 * Lines are given as in ocrs_engine_find_text_lines' output.  chars of line i
 * are (*chars)[char_offsets[i] .. char_offsets[i+1]); an empty range is the
 * reference's `None`.  char_offsets has n_lines+1 entries. */
OCRS_API ocrs_status ocrs_engine_recognize_text(const ocrs_engine* e, const ocrs_page* page, const float* line_rects,
                                       const size_t* line_offsets, size_t n_lines, ocrs_text_char** chars,
                                       size_t** char_offsets);
/* Batched form over several pages (lines of all pages share recognition
 * batches; padded widths stay those of recognition.rs:437).  page_line_offsets
 * has n_pages+1 entries indexing into line_offsets' line numbering. */
OCRS_API ocrs_status ocrs_engine_recognize_text_batch(const ocrs_engine* e, const ocrs_page* const* pages, size_t n_pages,
                                             const size_t* page_line_offsets, const float* line_rects,
                                             const size_t* line_offsets, size_t n_lines,
                                             ocrs_text_char** chars, size_t** char_offsets);

/* Recognition confidence (DESIGN.md "Recognition confidence"): the two calls above, plus
 *   char_logp:  one float per returned ocrs_text_char, same indexing: the log-prob of the CTC step the char came from
 *               (the masked log-prob the decoder saw; in greedy decoding the row's maximum);
 *   line_score: n_lines doubles: greedy, the log-probability of the greedy alignment path (sum over all T steps of
 *               the line, padding included, of the masked row maximum, in ascending t); beam search, the best
 *               beam's total.  A line without text (empty char range) has a score too; a line of no steps has 0.
 * Both malloc'ed (ocrs_buffer_free).  Scores say how sure the model was, not whether it is right: calibrate on real
 * models before thresholding. */
OCRS_API ocrs_status ocrs_engine_recognize_text_scored(const ocrs_engine* e, const ocrs_page* page, const float* line_rects,
                                                       const size_t* line_offsets, size_t n_lines, ocrs_text_char** chars,
                                                       size_t** char_offsets, float** char_logp, double** line_score);
OCRS_API ocrs_status ocrs_engine_recognize_text_batch_scored(const ocrs_engine* e, const ocrs_page* const* pages,
                                                             size_t n_pages, const size_t* page_line_offsets,
                                                             const float* line_rects, const size_t* line_offsets,
                                                             size_t n_lines, ocrs_text_char** chars, size_t** char_offsets,
                                                             float** char_logp, double** line_score);

/* Raw CTC output for the same lines (labels and time steps of
 * CtcHypothesis::steps(), recognition.rs:257-289), for token-level parity. */
OCRS_API ocrs_status ocrs_engine_recognize_tokens(const ocrs_engine* e, const ocrs_page* page, const float* line_rects,
                                         const size_t* line_offsets, size_t n_lines, uint32_t** labels,
                                         uint32_t** positions, size_t** token_offsets);

/* The recognition model's output for the same lines, before masking and decoding (TextRecognizer::run,
 * recognition.rs:341-360): line i owns rows [row_offsets[i], row_offsets[i+1]) of the [rows][classes] matrix *logp — its
 * T_i time steps.  One request, never coalesced.  For tolerance checks between numerics modes. */
OCRS_API ocrs_status ocrs_engine_recognize_logits(const ocrs_engine* e, const ocrs_page* page, const float* line_rects,
                                         const size_t* line_offsets, size_t n_lines, float** logp, size_t** row_offsets,
                                         int* classes);

/* Test hook: ops [first_op, last_op] of the recognition model (graph order, as in the model file) over n_lines lines of
 * model-input widths line_widths[i] (the model's input height), through the engine's own packed path — its options,
 * numerics, stream lease, ragged packing and launches.  `input`: op first_op's input, line after line in the per-line layout
 * of the graph ([H][W][C] NHWC in the conv stack and at the TOSEQ, [T][1][C] after it), input_len floats in all.  *out: op
 * last_op's output in the same layout, or with gx_only (last_op a GRU) that layer's input projections [2 directions][T][3H];
 * *out_offsets [n_lines + 1] float offsets of the lines in *out, *out_shapes [n_lines][3] their dims.  A range that starts
 * or ends inside a fused launch (conv1 + conv2 + pools, conv + pooled epilogue, average pool + TOSEQ) fails
 * (OCRS_ERR_INVALID_ARGUMENT) with the launch's bounds in ocrs_last_error().  Outputs are malloc'ed (ocrs_buffer_free). */
OCRS_API ocrs_status ocrs_engine_run_recognition_ops(const ocrs_engine* e, const int32_t* line_widths, size_t n_lines, int first_op,
                                                     int last_op, int gx_only, const float* input, size_t input_len, float** out,
                                                     size_t** out_offsets, int32_t** out_shapes);

/* TextItem::rotated_rect (text_items.rs:18-30) for a TextLine / TextWord given its characters'
 * rects (n x {top,left,bottom,right}): minimum-area rectangle of the box corners, oriented
 * towards "up" (y = -1).  out6 = (center.x, center.y, up.x, up.y, width, height).  Host side. */
OCRS_API ocrs_status ocrs_text_item_rotated_rect(const int32_t* rects_tlbr, size_t n_chars, float out6[6]);
/* RotatedRect::corners (order pinned by text_items.rs:156-166): out8 = 4 x (x, y). */
OCRS_API ocrs_status ocrs_rotated_rect_corners(const float rect6[6], float out8[8]);

/* OcrEngine::prepare_recognition_input (lib.rs:268-278 -> recognition.rs:366-392):
 * *out receives a [height, width] f32 line image. */
OCRS_API ocrs_status ocrs_engine_prepare_recognition_input(const ocrs_engine* e, const ocrs_page* page, const float* line,
                                                  size_t n_words, float** out, int* height, int* width);

/* ------------------------------------------------------------------------
 * Rectified line crops (no reference counterpart, opt-in).  The crop of the calls above takes the
 * axis-aligned bounding box of the line polygon, so a skewed line of width W and height h is cropped from a box of
 * height h + W |sin theta| and squeezed.  The _rectified calls crop every line along its own axis instead: the axis is the
 * least-squares line through the word centres (the first word's direction for one word or equal centre columns), the
 * frame the extent of the words' corners along and across it, and the crop a bilinear gather through an affine map,
 * masked per column to the rows its words span.  Everything after the crop — width groups, the model, decoding,
 * scores — is that of the plain calls.  Scope: skew that find_text_lines still groups into lines (a few tens of degrees).
 *
 * ocrs_line_frame (host only, no GPU): the frame of one line of n_words rects for a recogniser of input height
 * rec_height.  axis = (a.x, a.y); extents = (s_min, s_max, t_min, t_max), the corners' projections on a and on the normal
 * (-a.y, a.x); *resized_width = resized_line_width(ceil(s_max - s_min), ceil(t_max - t_min), rec_height); coef = the
 * map's (x0, ax, bx, y0, ay, by): output pixel (oy, ox) samples the page at X = (x0 + ax (ox + .5)) + bx (oy + .5), Y
 * likewise, in float32; ranges (optional, [n_words][4]) = every word's (c0, c1, r0, r1) of the mask, c0 > c1 for a word
 * that covers nothing.  *empty = 1 for a degenerate line (a value that is not finite, or a frame without width or height):
 * its crop is all -0.5 at the width the plain crop gives a bounding box with a side of zero, it has no char boxes, and
 * the other outputs are zero.
 * ocrs_line_char_boxes (host only): the page boxes of that line's chars from the CTC steps' positions (ascending) of a
 * model output of ctc_input_len steps: rects_tlbr [n_steps][4], kept [n_steps] (0: the char starts in the padding and is
 * dropped).  A char's box is the bounding box of its slice of the frame, so TextLine::rotated_rect and the JSON vertices
 * work from these as they do from the plain call's. */
OCRS_API ocrs_status ocrs_line_frame(const float* words, size_t n_words, int rec_height, double axis[2], double extents[4],
                                     uint32_t* resized_width, float coef[6], int32_t* ranges, int* empty);
OCRS_API ocrs_status ocrs_line_char_boxes(const float* words, size_t n_words, int rec_height, uint32_t ctc_input_len,
                                          const uint32_t* positions, size_t n_steps, int32_t* rects_tlbr, uint8_t* kept);
/* ocrs_engine_prepare_recognition_input / ocrs_engine_recognize_text[_batch] with rectified crops.  char_logp and
 * line_score: the outputs of the _scored calls, or both NULL.  One-page calls of both kinds may be merged into one batch
 * (option "coalesce"); each caller's lines are cropped its way and its results are those of its call alone. */
OCRS_API ocrs_status ocrs_engine_prepare_recognition_input_rectified(const ocrs_engine* e, const ocrs_page* page, const float* line,
                                                                     size_t n_words, float** out, int* height, int* width);
OCRS_API ocrs_status ocrs_engine_recognize_text_rectified(const ocrs_engine* e, const ocrs_page* page, const float* line_rects,
                                                          const size_t* line_offsets, size_t n_lines, ocrs_text_char** chars,
                                                          size_t** char_offsets, float** char_logp, double** line_score);
OCRS_API ocrs_status ocrs_engine_recognize_text_batch_rectified(const ocrs_engine* e, const ocrs_page* const* pages, size_t n_pages,
                                                                const size_t* page_line_offsets, const float* line_rects,
                                                                const size_t* line_offsets, size_t n_lines, ocrs_text_char** chars,
                                                                size_t** char_offsets, float** char_logp, double** line_score);
/* ocrs_engine_recognize_tokens over rectified crops: the raw CTC steps the char boxes come from. */
OCRS_API ocrs_status ocrs_engine_recognize_tokens_rectified(const ocrs_engine* e, const ocrs_page* page, const float* line_rects,
                                                            const size_t* line_offsets, size_t n_lines, uint32_t** labels,
                                                            uint32_t** positions, size_t** token_offsets);

/* ------------------------------------------------------------------------
 * Quarter turns and auto-orientation (no reference counterpart, opt-in).  find_text_lines groups words
 * along x, so a page that went through the feeder sideways or upside down reads as nothing.  These calls turn a resident
 * page by multiples of 90 degrees on the device, decide which turn makes it read, and map the results of the turned page
 * back to the frame of the page as given.  A turned page is an ordinary ocrs_page: every other call takes it.
 *
 * ocrs_engine_rotate_page[s]: *out = np.rot90(page, k), counter-clockwise: k = 1: out[i][j] = in[j][W-1-i] (shape
 * [W, H]), k = 2: out[i][j] = in[H-1-i][W-1-j], k = 3: out[i][j] = in[H-1-j][i] (shape [W, H]), k = 0: a copy.  Any
 * integer k, reduced to ((k % 4) + 4) % 4.  Pure data movement: every bit pattern survives.  out is a new page on the
 * page's device, independent of the source (also for k = 0); release both with ocrs_page_free in any order.  The batch
 * form turns n pages of any sizes by their own quarter_turns[i] in one launch; out[n] receives the pages.
 *
 * ocrs_unrotate_rects / ocrs_unrotate_chars (host only, in place): results found on rot90(page, k) mapped back to the
 * page_h x page_w page.  Coordinates are points of the pixel-index frame: k = 1: x = (W-1) - y', y = x', up = (-uy', ux');
 * k = 2: x = (W-1) - x', y = (H-1) - y', up = (-ux', -uy'); k = 3: x = y', y = (H-1) - x', up = (uy', -ux').  Widths and
 * heights are untouched.  Rects: float32, one subtraction from (float)(W-1) or (float)(H-1).  Char boxes: integers, the
 * four bounds mapped and swapped so that left <= right and top <= bottom stay true (k = 1: left = W-1-bottom',
 * right = W-1-top', top = left', bottom = right').
 *
 * ocrs_orientation_vote (host only): the word-shape vote over n word rects.  Per word, in order: its four corners as
 * ocrs_rotated_rect_corners gives them (float32), bw = max x - min x, bh = max y - min y; a word with a value, a corner or
 * an extent that is not finite is skipped; bw >= bh adds bw to out[0], else bh to out[1] (float64 sums).  The page reads
 * horizontally iff out[0] >= out[1] (also with no words).
 *
 * ocrs_engine_detect_orientation: which of the four quarter turns makes the page read.
 *   (a) detect_words on the page as given, then the vote: the candidates are {0, 2} if it reads horizontally, else {1, 3};
 *   (b) the candidates other than 0 are turned in one launch and detected as one batch (k = 0 keeps the words of (a));
 *   (c) find_text_lines per candidate; of each candidate up to max_lines lines (0 = all): those of the most words, ties to
 *       the lower line index, kept in line order;
 *   (d) one scored recognition batch over both candidates' lines (plain crops, the engine's decode method);
 *   (e) score[k] = (sum of the char log-probs, float64, in line order then char order) / n_chars[k]; -inf without chars;
 *       the two turns that are not candidates get NaN and n_chars 0;
 *   (f) *quarter_turns = the candidate of the larger score; a tie, and -inf twice, go to the smaller k.
 * Turn the page by *quarter_turns (ocrs_engine_rotate_page) to read it.  vote, score and n_chars may be NULL.  The
 * detection and recognition requests inside go the way of the public batch calls and may be merged with concurrent
 * one-page calls (option "coalesce").  The scores are the recognition confidence above: uncalibrated. */
OCRS_API ocrs_status ocrs_engine_rotate_page(const ocrs_engine* e, const ocrs_page* page, int quarter_turns, ocrs_page** out);
OCRS_API ocrs_status ocrs_engine_rotate_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* quarter_turns,
                                              ocrs_page** out);
OCRS_API ocrs_status ocrs_unrotate_rects(float* rects6, size_t n, int page_h, int page_w, int k);
OCRS_API ocrs_status ocrs_unrotate_chars(ocrs_text_char* chars, size_t n, int page_h, int page_w, int k);
/* "Page framing" above: results of a page cut out at (x0, y0) back in the frame of the page it was cut from */
OCRS_API ocrs_status ocrs_uncrop_rects(float* rects6, size_t n, int x0, int y0);
OCRS_API ocrs_status ocrs_uncrop_chars(ocrs_text_char* chars, size_t n, int x0, int y0);
/* "Page deskew" above: its char boxes (declared here, after ocrs_text_char). */
OCRS_API ocrs_status ocrs_unwarp_chars(ocrs_text_char* chars, size_t n, const float m[6]);
/* "Perspective correction" above: its char boxes. */
OCRS_API ocrs_status ocrs_unproject_chars(ocrs_text_char* chars, size_t n, const float m[8]);
OCRS_API ocrs_status ocrs_orientation_vote(const float* rects6, size_t n, double out[2]);
OCRS_API ocrs_status ocrs_engine_detect_orientation(const ocrs_engine* e, const ocrs_page* page, size_t max_lines, int* quarter_turns,
                                                    double vote[2], double score[4], uint32_t n_chars[4]);

/* OcrEngine::get_text (lib.rs:290-300): UTF-8, lines joined by '\n'. */
OCRS_API ocrs_status ocrs_engine_get_text(const ocrs_engine* e, const ocrs_page* page, char** text);

/* ------------------------------------------------------------------------
 * JPEG hand-off.  The reference decodes image files on the host with the `image` crate before
 * prepare_input (ocrs-cli/src/main.rs:312-333: image::open(path).into_rgb8()).  Here the host does only what is
 * inherently serial — marker parsing and Huffman entropy decoding, baseline / extended sequential and progressive —
 * and the GPU does dequantisation, the 8x8 inverse DCT, chroma upsampling and YCbCr -> RGB with libjpeg's integer
 * arithmetic (jidctint.c islow, jdsample.c fancy upsampling, jdcolor.c), so the pixels equal libjpeg-turbo's / PIL's
 * bit for bit; what crosses PCIe is the sparse coefficient stream (*coef_bytes, ~0.5-1 byte per pixel) instead of
 * 3 bytes per pixel.  Unsupported flavours (arithmetic coding, lossless, 12-bit, CMYK, 4:4:0 or exotic sampling) return
 * OCRS_ERR_IMAGE_SOURCE: decode those on the host as the reference does and call ocrs_engine_prepare_input.
 *   ocrs_engine_prepare_input_jpeg  OcrEngine::prepare_input(ImageSource::from_bytes(into_rgb8(decode(file)))) in one call
 *   ocrs_jpeg_decode_rgb            the decoded RGB8 HWC pixels on the host (tests, debugging); *rgb: ocrs_buffer_free
 *   ocrs_jpeg_info                  host only: dimensions, component count, progressive?, non-zero coefficients
 * coef_bytes and the out-parameters of ocrs_jpeg_info may be NULL.
 * ---------------------------------------------------------------------- */
OCRS_API ocrs_status ocrs_engine_prepare_input_jpeg(const ocrs_engine* e, const void* jpeg, size_t len, ocrs_page** out,
                                                    size_t* coef_bytes);
OCRS_API ocrs_status ocrs_jpeg_decode_rgb(int device, const void* jpeg, size_t len, uint8_t** rgb, int* height, int* width,
                                          size_t* coef_bytes);
OCRS_API ocrs_status ocrs_jpeg_info(const void* jpeg, size_t len, int* height, int* width, int* components, int* progressive,
                                    size_t* nonzero);
/* Test hook (host only): what the host half hands to the GPU, dense.  geom = {width, height, components, hmax, vmax,
 * progressive, ycc} + per component {h, v, tq, width, height, blocks_w, blocks_h}; quant = 4 tables x 64, natural order;
 * *coef = n_blocks x 64 quantised coefficients in natural order, blocks in component order, row-major (ocrs_buffer_free). */
OCRS_API ocrs_status ocrs_jpeg_coefficients(const void* jpeg, size_t len, int32_t geom[28], uint16_t quant[256], int16_t** coef,
                                            size_t* n_blocks);

/* ------------------------------------------------------------------------
 * Several GPUs in one process: an engine group.  One engine (and one replica of the weights) per member device;
 * every page of a call is processed by a member of the device the page lives on, every member runs its share on a
 * worker thread and streams of its own, results come back in page order.  Pages are independent (OcrEngine is
 * immutable `&self`, ocrs/src/lib.rs:183-256), so there is no collective on the compute path; the only exchange is
 * the gather of the packed results, by one of two transports that deliver the same bytes:
 *   OCRS_GATHER_HOST  every member hands its results over through its own pinned staging / PCIe link and the calling
 *                     thread concatenates them
 *   OCRS_GATHER_RCCL  the packed results ({rect f32 x 6} per word, {char, box} per character), prefixed by their
 *                     length, are all-gathered device to device over xGMI (ncclCommInitAll communicator, one grouped
 *                     ncclAllGather) and read back from the root member
 *   OCRS_GATHER_AUTO  for ocrs_group_params.gather (the per-request gathers inside ocrs_group_detect_words_batch /
 *                     ocrs_group_recognize_text_batch): host — inside one process the results are on the host
 *                     already.  For ocrs_group_final_gather (the end-of-stream gather; north_star: "RCCL over xGMI
 *                     only for the final result gather"): RCCL when the group has two or more members and a
 *                     communicator can be had, else host.
 * librccl is loaded at run time (dlopen: `librccl.so.1`, or what OCRS_RCCL_LIB names) by the first gather that asks for
 * it; libocrs_amd.so itself does not depend on it.  RCCL not loadable, a communicator refused (RCCL does not accept the
 * same device twice: a group such as [0, 0] on a one-GPU box) — every such case falls back to the host transport and
 * ocrs_group_last_gather reports it; none is an error.
 *
 * Dealing.  Pages the caller made resident (ocrs_group_prepare_input_device_batch; ocrs_page handles) stay where they
 * are.  Pages the group places itself (ocrs_group_prepare_input_batch) go to the devices in contiguous blocks of
 * ceil(n / devices) pages, but at least `group_min_block` (option, default 8): a call of 16 pages on 8 devices uses
 * two of them, and successive calls start at successive devices — a device handed two pages runs its batch kernels
 * at a fraction of their efficiency.  Members that share a device split its pages the same way in blocks of at
 * least `group_shared_block` (16).  ocrs_group_deal is the block rule on its own, starting at member 0.
 * ---------------------------------------------------------------------- */
typedef struct ocrs_engine_group ocrs_engine_group;
typedef enum ocrs_gather_mode { OCRS_GATHER_AUTO = 0, OCRS_GATHER_HOST = 1, OCRS_GATHER_RCCL = 2 } ocrs_gather_mode;

typedef struct ocrs_group_params { /* OcrEngineParams (lib.rs:38-71) + the member devices */
    const void* detection_model;   /* `.ocrsm` image (as for ocrs_model_load_bytes) or NULL */
    size_t detection_model_len;
    const void* recognition_model;
    size_t recognition_model_len;
    const int* devices;            /* member m runs on devices[m] */
    size_t n_devices;
    int debug;
    ocrs_decode_method decode_method;
    uint32_t beam_width;
    const char* alphabet;
    const char* allowed_chars;
    ocrs_gather_mode gather;
    ocrs_numerics numerics;        /* as in ocrs_engine_params, for every member */
    int coalesce, coalesce_pages, coalesce_window_us, layout_threads;
    int64_t rec_max_pixels;
    int min_block;                 /* pages the group places itself go to a device in contiguous blocks of at least this
                                    * many (0 = default 8; a small call then uses fewer devices, successive calls rotate) */
    int shared_block;              /* the same between members that share one device (0 = default 16) */
} ocrs_group_params;

OCRS_API ocrs_status ocrs_engine_group_new(const ocrs_group_params* params, ocrs_engine_group** out);
OCRS_API void ocrs_engine_group_free(ocrs_engine_group* g);
OCRS_API ocrs_status ocrs_engine_group_size(const ocrs_engine_group* g, size_t* n_members);
/* Member i's engine (borrowed; usable with every ocrs_engine_* call) and device. */
OCRS_API ocrs_status ocrs_engine_group_member(const ocrs_engine_group* g, size_t i, const ocrs_engine** engine, int* device);
/* The dealing rule on its own (host only): block = max(ceil(n_pages / n_members), min(min_block, n_pages)) with
 * min_block = 0 meaning the default 8, member_of_page[i] = (i / block) mod n_members; pages_per_member may be NULL. */
OCRS_API ocrs_status ocrs_group_deal(size_t n_pages, size_t n_members, size_t min_block, size_t* member_of_page, size_t* pages_per_member);

/* OcrEngine::prepare_input (lib.rs:183-187) for n equally sized host images, dealt as described above.  out[n]
 * receives the pages (each lives on its member's device). */
OCRS_API ocrs_status ocrs_group_prepare_input_batch(const ocrs_engine_group* g, const void* const* pixels, size_t n,
                                                    ocrs_pixel_type type, ocrs_dim_order order, int height, int width,
                                                    int channels, ocrs_page** out);
/* The same with the images already resident on member devices (ocrs_device_malloc_on): each is converted where it is. */
OCRS_API ocrs_status ocrs_group_prepare_input_device_batch(const ocrs_engine_group* g, const void* const* d_pixels, size_t n,
                                                           ocrs_pixel_type type, ocrs_dim_order order, int height, int width,
                                                           int channels, ocrs_page** out);
/* OcrEngine::detect_words (lib.rs:193-199); every page is processed on the device it lives on (which must have a
 * member); output as ocrs_engine_detect_words_batch. */
OCRS_API ocrs_status ocrs_group_detect_words_batch(ocrs_engine_group* g, const ocrs_page* const* pages, size_t n_pages,
                                                   float** rects, size_t* offsets);
/* The same with detection confidence; output as ocrs_engine_detect_words_batch_scored.  Scores and pixel counts travel in
 * the per-request payload next to the rects, through either gather transport. */
OCRS_API ocrs_status ocrs_group_detect_words_batch_scored(ocrs_engine_group* g, const ocrs_page* const* pages, size_t n_pages,
                                                          float** rects, size_t* offsets, float** score, uint32_t** pixels);
/* Tiled detection (ocrs_engine_detect_words_batch_tiled) with every page on the member of its device; score and pixels may
 * both be NULL.  Results are gathered as the scored call gathers them. */
OCRS_API ocrs_status ocrs_group_detect_words_batch_tiled(ocrs_engine_group* g, const ocrs_page* const* pages, size_t n_pages, int overlap,
                                                         float** rects, size_t* offsets, float** score, uint32_t** pixels);
/* OcrEngine::recognize_text (lib.rs:237-256); arguments and output as ocrs_engine_recognize_text_batch.
 * (find_text_lines is host work: ocrs_engine_find_text_lines_batch serves a group as it is.) */
OCRS_API ocrs_status ocrs_group_recognize_text_batch(ocrs_engine_group* g, const ocrs_page* const* pages, size_t n_pages,
                                                     const size_t* page_line_offsets, const float* line_rects,
                                                     const size_t* line_offsets, size_t n_lines, ocrs_text_char** chars,
                                                     size_t** char_offsets);
/* The same with rectified crops (ocrs_engine_recognize_text_batch_rectified); not recorded by the replay mode. */
OCRS_API ocrs_status ocrs_group_recognize_text_batch_rectified(ocrs_engine_group* g, const ocrs_page* const* pages, size_t n_pages,
                                                               const size_t* page_line_offsets, const float* line_rects,
                                                               const size_t* line_offsets, size_t n_lines, ocrs_text_char** chars,
                                                               size_t** char_offsets);
/* The per-request gather on its own: payloads[m] / bytes[m] = member m's packed bytes (host memory); *out receives
 * their concatenation in member order through the group's per-request transport, offsets[G + 1] the boundaries. */
OCRS_API ocrs_status ocrs_group_gather(ocrs_engine_group* g, const void* const* payloads, const size_t* bytes, void** out,
                                       size_t* offsets);
/* The final result gather of a stream of requests: the same contract with the transport named per call (AUTO = RCCL
 * when the group has two or more members and RCCL can be had, else host — never an error for lack of RCCL). */
OCRS_API ocrs_status ocrs_group_final_gather(ocrs_engine_group* g, ocrs_gather_mode mode, const void* const* payloads,
                                             const size_t* bytes, void** out, size_t* offsets);
/* Test hook — host-side pre-flight of a multi-GPU deployment on a box with fewer GPUs (bench.py --replay; SURVEY §8e names the
 * host as the expected scaling limiter).  mode 1 = record: calls run as usual and the group keeps every page's word rects and
 * recognised lines, keyed by the host pixels the page was prepared from (ocrs_group_prepare_input_batch).  mode 2 = replay: a
 * member's share of a call does no GPU work — it sleeps seconds[stage] (stage 0 prepare, 1 detect, 2 recognize: what one
 * share takes on one GPU under load) and returns the recorded results of its pages — while dealing, worker threads and their
 * NUMA binding, payload packing, the per-request and final gathers and the reassembly in page order run as in production.
 * mode 0 = off (forgets the records).  Not for concurrent use with calls in flight. */
OCRS_API ocrs_status ocrs_group_set_replay(ocrs_engine_group* g, int mode, const double seconds[3]);
/* What member m has done so far, for diagnosing a multi-GPU run (the host side is the expected scaling
 * limiter): out = {shares of calls it ran, pages those carried, CPU nanoseconds of the host threads that ran them, their wall
 * nanoseconds, NUMA node of its GPU + 1 (0 = the host does not say), CPUs of that node (0 = no binding), shares that ran
 * bound to those CPUs, its device}.  A member's share of a call binds its thread to the CPUs of the NUMA node the member's
 * GPU hangs off (hipDeviceGetPCIBusId -> sysfs numa_node / cpulist) for the duration of the share and restores the thread's
 * mask afterwards; its page-locked staging is first touched from there.  Hosts without that information: no binding. */
OCRS_API ocrs_status ocrs_group_member_stats(const ocrs_engine_group* g, size_t m, uint64_t out[8]);
/* Host-only helpers behind that placement, exported for tests: a sysfs cpu list ("0-3,8") parsed into cpu numbers (cpus may
 * be NULL; *n_cpus = how many the list names); and: node of a PCI device under `sysfs_root` (NULL = "/sys"), the calling
 * thread bound to that node's CPUs inside a scope (*cpus_inside = CPUs in its mask there, -1 = not bound) and restored
 * (*cpus_after). */
OCRS_API ocrs_status ocrs_numa_parse_cpulist(const char* list, int32_t* cpus, size_t capacity, size_t* n_cpus);
OCRS_API ocrs_status ocrs_numa_bind_selftest(const char* sysfs_root, const char* pci_bus_id, int* node, int* cpus_inside, int* cpus_after);
/* Worker threads the group has created so far (they are kept between calls). */
OCRS_API ocrs_status ocrs_group_worker_threads(const ocrs_engine_group* g, size_t* n);
/* Transport of the group's most recent gather: 1 host, 2 RCCL (0: none yet), the payload bytes it moved, and — when it
 * used the host transport — why (valid until the next call of this function on the group; "" otherwise).  Any
 * argument may be NULL. */
OCRS_API ocrs_status ocrs_group_last_gather(const ocrs_engine_group* g, int* transport, size_t* bytes, const char** why_host);

/* ------------------------------------------------------------------------
 * Measurement hooks (bench.py; not part of the reference surface).
 * ---------------------------------------------------------------------- */
/* Device memory helpers so that bench inputs can be made HBM-resident without
 * torch in the loop.  free / upload take pointers of any device. */
OCRS_API ocrs_status ocrs_device_malloc(size_t bytes, void** d_ptr);                 /* on the default device */
OCRS_API ocrs_status ocrs_device_malloc_on(int device, size_t bytes, void** d_ptr);
OCRS_API ocrs_status ocrs_device_free(void* d_ptr);
OCRS_API ocrs_status ocrs_device_upload(void* d_dst, const void* h_src, size_t bytes);
OCRS_API ocrs_status ocrs_device_synchronize(void);
/* Page-locked host memory: ocrs_engine_prepare_input{,_batch} from such a buffer is a DMA transfer that overlaps
 * GPU work (from ordinary memory the runtime stages every copy through a bounce buffer).  An image decoder that
 * writes its output here hands pages over at PCIe speed. */
OCRS_API ocrs_status ocrs_host_malloc(size_t bytes, void** h_ptr);
OCRS_API ocrs_status ocrs_host_free(void* h_ptr);
/* Rates this device sustains: register-only fp32 MFMA loop (TFLOP/s) and a large float4 copy
 * (GB/s, read + write).  Reported by bench.py beside the nominal peaks the roofline uses. */
OCRS_API ocrs_status ocrs_device_measure_peaks(double* mfma_f32_tflops, double* hbm_copy_gbps);

/* Per-stage timers: when enabled, every GPU stage is bracketed by HIP events
 * on the stream it is launched on; ocrs_engine_stage_times returns accumulated
 * milliseconds and launch counts since the last reset.  Stage names:
 * ocrs_stage_name(i), i < ocrs_stage_count(). */
OCRS_API ocrs_status ocrs_engine_enable_timing(ocrs_engine* e, int enable); /* 0 off, 1 stages, 2 stages + kernels */
OCRS_API int ocrs_stage_count(void);
OCRS_API const char* ocrs_stage_name(int stage);
OCRS_API ocrs_status ocrs_engine_stage_times(ocrs_engine* e, double* ms, uint64_t* launches, int reset);

/* Kernel-class timers of the model executor (enable_timing(e, 2)): every launch
 * is bracketed by HIP events on its stream; flops/bytes are the ALGORITHMIC
 * figures of DESIGN.md §6 summed over the launches. */
/* Restrict per-launch kernel timing to the classes whose bit is set (default: all). */
OCRS_API ocrs_status ocrs_engine_set_kernel_timing_mask(ocrs_engine* e, uint32_t mask);
/* Request coalescing (ocrs_engine_params.coalesce): {merged batches run, caller requests they carried} per stage since the engine
 * was created.  requests > batches means calls of different host threads shared launches. */
OCRS_API ocrs_status ocrs_engine_coalesce_stats(const ocrs_engine* e, uint64_t detect[2], uint64_t recognize[2]);
OCRS_API int ocrs_kernel_class_count(void);
OCRS_API const char* ocrs_kernel_class_name(int cls);
OCRS_API ocrs_status ocrs_engine_kernel_stats(ocrs_engine* e, double* ms, uint64_t* launches, double* flops,
                                              double* bytes, int reset);
/* Per class, the part of `flops` that ran on the matrix cores (all of it for the gemm_*_mfma classes; the pointwise
 * convolutions and ConvTranspose of a fused detection block when its MFMA variant ran).  Call BEFORE a resetting
 * ocrs_engine_kernel_stats. */
OCRS_API ocrs_status ocrs_engine_kernel_mfma_flops(ocrs_engine* e, double* mfma_flops);

#ifdef __cplusplus
}
#endif
#endif /* OCRS_AMD_H */
