// Launch wrappers for every HIP kernel in libocrs_amd (gfx950).  All take the
// stream to launch on; none synchronises.  Activations are NHWC fp32.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ocrs {
namespace jpeg { struct Coefficients; }
namespace k {

// ---- kernels_image.hip ----------------------------------------------------
// prepare_image (preprocess.rs:149-248): pixels -> grey f32 [H,W] in [-0.5,0.5].
void prepare_image(const void* d_pixels, bool is_u8, bool chans_last, int h, int w, int chans, float* d_out,
                   hipStream_t s);
// The same for the n pages of one call, all h x w of one format, in one launch per PrepareTable::kPages pages: the
// descriptor table (source and destination of each page) travels in the kernel's arguments.  Same bits as prepare_image.
struct PrepareTable {
    enum { kPages = 32 };
    const void* src[kPages];
    float* dst[kPages];
};
void prepare_image_batch(const void* const* d_pixels, float* const* d_out, int n, bool is_u8, bool chans_last, int h, int w,
                         int chans, hipStream_t s);
// pad(-0.5) + bilinear resize of N equally sized pages to the model input
// (detection.rs:155-171).  src_ptrs: device array of N page pointers [sh,sw].
void resize_pages_to_model(const float* const* d_src_ptrs, int n, int sh, int sw, int vh, int vw, float* d_dst,
                           int dh, int dw, hipStream_t s);
// slice + bilinear resize back + strict threshold (detection.rs:187-194,110).
// prob: [n, mh, mw] (only the top-left [sh, sw] is read); mask: [n, h, w] u8;
// d_map (optional, may be null): [n, h, w] f32 probability map.
// d_labels / d_zero_a / d_zero_b (optional, r6): the component stage's label array [n, h, w] and its two per-page counters
// (CclBuffers::overflow, ::offsets).  When all three are given and the shapes allow (w % 4 == 0, aligned buffers, option
// ccl_quad) the launch also writes the initial labels and zeroes the counters, and returns true: ccl_label and contour_rects
// are then told to skip their first step (`prepared`).
bool resize_threshold(const float* d_prob, int n, int mh, int mw, int sh, int sw, float thr, uint8_t* d_mask,
                      float* d_map, int h, int w, hipStream_t s, int32_t* d_labels = nullptr, int32_t* d_zero_a = nullptr,
                      int32_t* d_zero_b = nullptr);
void threshold_only(const float* d_prob, float thr, uint8_t* d_mask, int64_t count, hipStream_t s);

// ---- kernels_ccl.hip ------------------------------------------------------
struct CclBuffers {
    int32_t* labels;      // [n, h, w]
    int32_t* row_counts;  // [n, h]
    int32_t* row_offsets; // [n, h]
    int32_t* n_roots;     // [n]  external components per page
    int32_t* roots;       // [n, max_comp]  raster-ordered start pixels
    int32_t* lengths;     // [n, max_comp]  (unused since r3: lengths are found by the contour kernel itself)
    int32_t* offsets;     // [n]            per-page bump counter of the contour arena
    int32_t* overflow;    // [n]  set if a capacity was exceeded
    uint32_t* pts;        // [n, arena]  packed (y << 16 | x) contour points
    uint32_t* tmp;        // [n, 4 * arena]  per component: simplified | sorted | hull (2x) scratch
    uint8_t* keep;        // [n, arena]
    float* rects;         // [n, max_comp, 6]
    uint8_t* valid;       // [n, max_comp]
    uint32_t* score_pixels;            // [n, max_comp]  scored requests only (else null): pixels of the slot's component
    unsigned long long* score_sums;    // [n, max_comp]  ... and the sum of floor(clamp(p, 0, 1) * 2^24) over them
};
// mask [n,h,w] -> per page: raster-ordered external components -> rects
// (find_contours(External) -> simplify_polygon(2) -> min_area_rect -> resize(+2*expand)
//  -> area >= min_area; detection.rs:41-62).
// prepared: resize_threshold already wrote the initial labels / zeroed the counters (it returned true)
void ccl_label(const uint8_t* d_mask, int n, int h, int w, const CclBuffers& b, int max_comp, hipStream_t s, bool prepared = false);
void contour_rects(const uint8_t* d_mask, int n, int h, int w, const CclBuffers& b, int max_comp, int64_t arena,
                   float expand, float min_area, float eps, hipStream_t s, bool prepared = false);

// (kernels_score.hip)  Per slot of b.roots: the component's pixel count and fixed-point probability sum, into b.score_pixels /
// b.score_sums (zeroed here).  After ccl_label, on its stream; d_map: the page-resolution probabilities [n, h, w] the mask
// was thresholded from.  A page whose roots overflowed max_comp is left at zero (it is re-run, like its rects).
void component_scores(const uint8_t* d_mask, const float* d_map, int n, int h, int w, const CclBuffers& b, int max_comp,
                      hipStream_t s);

// ---- kernels_tile.hip: tiled detection --------------------
struct TileDesc {          // one model-sized tile of a page, cut at the page's own resolution
    const float* page;     // [h, w] grey page
    uint8_t* mask;         // [h, w] the page's text mask
    float* map;            // [h, w] the page's probability map, or null
    int32_t h, w;
    int32_t oy, ox;        // tile origin in the page
    int32_t y0, y1, x0, x1;   // the page pixels this tile owns: oy <= y0 < y1 <= min(oy + mh, h), likewise x
};
// d_dst[t] = the [mh, mw] model input of tile t: page[oy + r, ox + c] inside the page, -0.5 outside; tiles of any mix of pages
void gather_tiles(const TileDesc* d_tiles, int n_tiles, float* d_dst, int mh, int mw, hipStream_t s);
// d_prob [n_tiles, mh, mw]: every tile writes the pixels it owns: mask = p > thr (strict) and, where map is set, p
void stitch_threshold(const TileDesc* d_tiles, int n_tiles, const float* d_prob, int mh, int mw, float thr, hipStream_t s);

// ---- kernels_nn.hip -------------------------------------------------------
// C[M,N] = act(A[M,K] . B[K,N] + bias[N]) as an exact fp32 MFMA chain, k ascending.
struct GemmDesc {
    const float* A; int lda;      // dense: row-major [M][lda]
    const float* B; int ldb;      // row-major [K][ldb]
    const float* bias;            // [N] (may be null -> 0)
    float* C; int ldc;
    int M, N, K;
    int relu;
    // im2col (3x3, pad 1) view of an NHWC tensor [n, H, W, Cin]: M = n*H*W, K = 9*Cin
    int im2col; int H, W, Cin;
    // ConvTranspose2x2/s2 scatter epilogue: rows are input pixels [n,H,W], columns (dy,dx,co)
    int convt; int Cout;
    // batched (blockIdx.z) strides, elements
    int batch; int64_t strideA, strideB, strideBias, strideC;
    // set by the launcher (gemm_tiled, dense A): 1-D grid, the column tiles of a row tile run side by side on one XCD
    int nfast = 0, nx = 0, ny = 0;
    // relaxed / reduced numerics: B cut into bf16 terms (split_mfma.hpp split_weights), per batch strideBsplit uint16 apart; or null
    const uint16_t* Bsplit = nullptr; int64_t strideBsplit = 0;
};
void gemm(const GemmDesc& d, hipStream_t s);
// Direct conv (k x k, same padding, Cout % 4 == 0) for tiny contractions / odd shapes.
void conv_direct(const float* x, int n, int h, int w, int cin, const float* wt, const float* bias, int kh, int kw,
                 int cout, int relu, float* y, hipStream_t s);
void dwconv3x3(const float* x, int n, int h, int w, int c, const float* wt, const float* bias, int relu, float* y,
               hipStream_t s);
// dw 3x3 + pw 1x1 in one pass (8 <= C <= 32); same arithmetic as the two separate kernels
bool dwpw_fused_supported(int cin, int cout);
void dwpw_fused(const float* x, int n, int h, int w, int cin, const float* wdw, const float* bdw, int relu_dw, int cout,
                const float* wpw, const float* bpw, int relu_pw, float* y, hipStream_t s);
// depthwise 3x3 over concat([skip, centred-pad(up)]) without building the concatenation; false if unsupported
bool dwconv3x3_cat(const float* skip, int n, int h, int w, int cs, const float* up, int uh, int uw, int cu, const float* wt,
                   const float* bias, int relu, float* y, hipStream_t s);
// ---- kernels_det.hip: a whole DoubleConv block of the detection U-Net in one launch (LDS halo tiles):
//   [cat(skip, pad(ConvT2x2/s2(x1)))] -> dw3x3 -> pw1x1 -> dw3x3 -> pw1x1 -> y  [-> maxpool 2x2 | -> conv1x1(->1) -> sigmoid]
struct DoubleConvArgs {
    const float* skip;            // [n,h,w,CS]; encoder: the block input
    const float* x1;              // decoder: [n,h1,w1,CX] input of the ConvTranspose (else null)
    const float *wt, *bt;         // ConvT [2][2][CX][CS], [CS]
    const float *wd1, *bd1;       // dw1 [3][3][CIN], [CIN]   (CIN = CS, or 2*CS for a decoder block)
    const float *wp1, *bp1;       // pw1 [CIN][CMID], [CMID]
    const float *wd2, *bd2;       // dw2 [3][3][CMID], [CMID]
    const float *wp2, *bp2;       // pw2 [CMID][COUT], [COUT]
    const float *wf, *bf;         // final 1x1 conv [COUT], [1]
    float* y;                     // [n,h,w,COUT], or [n,h,w,1] with the final conv
    float* ypool;                 // [n,h/2,w/2,COUT] or null
    int n, h, w, h1, w1;
    int relu_d1, relu_p1, relu_d2, relu_p2, sigmoid;
    int tiles_x, tiles_y;         // filled by the launcher
    const float* tape = nullptr;  // wave streaming kernels (kernels_det_stream.hip): the block's weight tape(s) on the device
    int tape_len = 0;             // floats per tape
    const float* rtape = nullptr; // workgroup streaming kernels (kernels_det_rows.hip): the four waves' tapes
    int rtape_len = 0;
};
// host pointers to a block's weights, for building its tape
struct StreamWeights {
    const float *wt, *bt, *wd1, *bd1, *wp1, *bp1, *wd2, *bd2, *wp2, *bp2, *wf, *bf;
};
// true if a fused kernel exists for the shape (cs skip channels, cx ConvT input channels or 0, ...); launches it when
// `launch` is set.  *on_mfma: the block's pointwise convs / ConvTranspose run on the matrix cores.
// *path: which kernel family takes the shape with the current options and this request (a.n, a.h, a.w): 0 = LDS-tiled
// block, 1 = row-streaming wave kernel, 2 = row-streaming workgroup kernel.
bool double_conv_fused(const DoubleConvArgs& a, int cs, int cx, int cmid, int cout, bool pool, bool final_conv,
                       bool launch, hipStream_t s, bool* on_mfma = nullptr, int* path = nullptr);
// ---- kernels_det_stream.hip (r4): the same blocks as row-streaming register kernels for the full-resolution levels;
// true if the shape has one (launches it when `launch` is set).  Same bits as the tiled blocks and the per-op kernels.
// With `hw` / `tape_out` the block's weight tape is built (the weights in the order a row step consumes them; the caller
// uploads it and passes it in DoubleConvArgs::tape); *tape_len = floats per tape.
bool double_conv_stream(const DoubleConvArgs& a, int cs, int cx, int cmid, int cout, bool pool, bool final_conv, bool launch, hipStream_t s,
                        const StreamWeights* hw = nullptr, std::vector<float>* tape_out = nullptr, int* tape_len = nullptr);
// ---- kernels_det_rows.hip (r4): the blocks of the 16-64-channel levels as row-streaming workgroup kernels; same contract
// (the tape holds the four waves' depthwise weights).  At launch time false also when the geometry does not fit (then the
// tiled block runs).
bool double_conv_rows(const DoubleConvArgs& a, int cs, int cx, int cmid, int cout, bool pool, bool final_conv, bool launch, hipStream_t s,
                      const StreamWeights* hw = nullptr, std::vector<float>* tape_out = nullptr, int* tape_len = nullptr);
// the launch-time conditions of double_conv_rows (request size under option value 1, geometry): true if it will run
bool double_conv_rows_takes(const DoubleConvArgs& a, int cx);
void maxpool(const float* x, int n, int h, int w, int c, int kh, int kw, float* y, hipStream_t s);
void avgpool(const float* x, int n, int h, int w, int c, int kh, int kw, float* y, hipStream_t s);
void padcat(const float* skip, int n, int sh, int sw, int cs, const float* x, int h, int w, int cx, float* y,
            hipStream_t s);
void sigmoid(const float* x, float* y, int64_t count, hipStream_t s);
// pointwise conv with Cout == 1 (+ optional ReLU, then optional sigmoid): y[p] = act(b + sum_c x[p,c] w[c])
void conv1x1_cout1(const float* x, int64_t pixels, int cin, const float* wt, const float* bias, int relu, int do_sigmoid,
                   float* y, hipStream_t s);
// [N,1,W,C] -> [W,N,C]
void to_seq(const float* x, int n, int w, int c, float* y, hipStream_t s);
// GRU gates for one time step, both directions (grid.z = dir).
// gx: [2][T*N][3H] (dir-major), gh: [2][N][3H], h: [2][N][H], y: [T][N][2H].
void gru_gates(const float* gx, const float* gh, float* h, float* y, int T, int N, int H, int step, hipStream_t s);
// log_softmax over C (+ optional -inf masking of excluded labels) + argmax.
// logits/logp: [rows][C]; labels: [rows] (first max).  logp may be null.  maxlp (optional): [rows] the masked
// maximum itself.  Returns false (nothing launched) if C is too large for the kernel's LDS staging (more than ~630 classes).
bool log_softmax_argmax(const float* logits, int64_t rows, int c, const uint8_t* d_excluded /*[C] or null*/,
                        float* logp, int32_t* labels, hipStream_t s, float* maxlp = nullptr);
// Ragged sequence batch (lines sorted by length, rows off[t] + m); see kernels_nn.hip.
void to_seq_packed(const float* x, int n, int T, int c, const int32_t* d_pos, const int32_t* d_off, float* y,
                   hipStream_t s);
void gru_gates_packed(const float* gx, const float* gh, float* h, float* y, const int32_t* d_Tm, const int32_t* d_off,
                      int64_t R, int Mcap, int active, int H, int step, hipStream_t s);
// Fused recurrent step (hidden GEMM on 16x16x4 fp32 MFMA + gates), both directions.
// hT_in/hT_out: [2][H][Mcap] transposed state (Mcap % 4 == 0), ping-ponged by the caller.
bool gru_step_fused(const float* gx, const float* wh, const float* bh, const float* hT_in, float* hT_out, float* y,
                    const int32_t* d_Tm, const int32_t* d_off, int64_t R, int Mcap, int active, int H, int step,
                    hipStream_t s);
// ---- kernels_gru.hip: all time steps of one bidirectional GRU layer in ONE persistent launch.
// d_sync: gru_persistent_sync_words(M) words of scratch (zeroed by the call); its last word is non-zero
// afterwards if a wait inside the kernel timed out.  Returns false (nothing launched) if the shape is not
// supported (H, more than 4096 lines, Tmax beyond the LDS table, a device that cannot keep a whole group of clusters
// resident): the caller then runs gru_step_fused per step.
// hx: gru_persistent_exchange_bytes() of scratch, the hand-off buffer between the workgroups; gru_persistent_prepare marks
// every word of it "unwritten" (the data is its own flag); call it on a stream ordered before gru_persistent.
size_t gru_persistent_sync_words(int M);
size_t gru_persistent_exchange_bytes(const int32_t* h_Tm, int M, int H);
bool gru_persistent_supported(const int32_t* h_Tm, int M, int Tmax, int64_t R, int H);
bool gru_tile_plan(const int32_t* h_Tm, int M, int H, int* ncl, int* waves, int16_t* tiles /* [512] */);  // host only: the deal of row tiles to waves
hipError_t gru_persistent_prepare(float* hx, const int32_t* h_Tm, int M, int H, hipStream_t s);
// h_Tm: the same lengths as d_Tm on the host (descending) — the deal of row tiles to waves is computed from them.
bool gru_persistent(const float* gx, const float* wh, const float* bh, float* y, float* hx, const int32_t* d_Tm, const int32_t* d_off,
                    const int32_t* h_Tm, int64_t R, int M, int Tmax, int H, uint32_t* d_sync, hipStream_t s);
bool gru_general_tile_plan(const int32_t* h_Tm, int M, int Tmax, int H, int cap, int* ncl, int16_t* tiles /* [512] or null */, int kernel /* 0 fp32, 1 / 2: split with 3 / 2 planes */);
// ---- kernels_gru_split.hip: the same launch for numerics != exact: hidden contraction on the bf16 matrix cores with the state
// cut into np (2: reduced, 3: relaxed) bf16 planes.  hx: gru_split_exchange_bytes() of scratch, marked by gru_split_prepare on a
// stream ordered before; y needs no marks.  d_sync as above.
size_t gru_split_exchange_bytes(const int32_t* h_Tm, int M, int H, int np);
bool gru_split_supported(const int32_t* h_Tm, int M, int Tmax, int64_t R, int H, int np);
hipError_t gru_split_prepare(uint16_t* hx, const int32_t* h_Tm, int M, int H, int np, hipStream_t s);
bool gru_persistent_split(const float* gx, const float* wh, const float* bh, float* y, uint16_t* hx, const int32_t* d_Tm, const int32_t* d_off,
                          const int32_t* h_Tm, int64_t R, int M, int Tmax, int H, int np, uint32_t* d_sync, hipStream_t s);
void ctc_collapse_packed(const int32_t* labels, const int32_t* d_Tm, const int32_t* d_off, int M, int Tmax,
                         uint32_t* out_labels, uint32_t* out_pos, int32_t* out_count, hipStream_t s);
// ctc_collapse_packed plus confidence: out_logp [M][Tmax] each step's maxlp, out_score [M] the float64 sum of maxlp over
// the line's rows in ascending t (the greedy path's log-probability)
void ctc_collapse_scored_packed(const int32_t* labels, const float* maxlp, const int32_t* d_Tm, const int32_t* d_off, int M,
                                int Tmax, uint32_t* out_labels, uint32_t* out_pos, float* out_logp, int32_t* out_count,
                                double* out_score, hipStream_t s);
void argmax_rows(const float* x, int64_t rows, int c, const uint8_t* d_excluded, int32_t* labels, hipStream_t s);
// ---- kernels_beam.hip: CTC prefix beam search (rten decode_beam) on the packed log-probabilities, one workgroup
// per line; same results as the host's ctc_beam_search.  d_nodes / d_posn: M * ctc_beam_arena_entries(Tmax, width)
// int2 each (scratch).  Outputs in the layout of ctc_collapse_packed.  false if (C, width) is not supported.
// out_score (optional): [M] the best beam's lse(pb, pnb); out_logp (optional): [M][Tmax] each step's masked log-prob.
bool ctc_beam_supported(int C, int width);
size_t ctc_beam_arena_entries(int Tmax, int width);
bool ctc_beam_packed(const float* logp, const int32_t* d_Tm, const int32_t* d_off, int M, int Tmax, int C, int width,
                     const uint8_t* d_excluded, int2* d_nodes, int2* d_posn, uint32_t* out_labels, uint32_t* out_pos,
                     int32_t* out_count, hipStream_t s, double* out_score = nullptr, float* out_logp = nullptr);
// Greedy CTC collapse (rten decode_greedy): labels [T][N] -> per line (label,pos) lists.
void ctc_collapse(const int32_t* labels, int T, int N, uint32_t* out_labels, uint32_t* out_pos, int32_t* out_count,
                  hipStream_t s);

// ---- kernels_rec.hip: ragged batch of the recognition conv stack -----------
// All width groups of one request in one NHWC buffer: group-major, then image, y, x.
struct RaggedView {          // device pointers live in one metadata upload; passed by value
    int G;                   // groups
    int H;                   // image height at this layer (same for every group)
    const int32_t* W;        // [G] image width at this layer
    const int32_t* n;        // [G] images per group
    const int64_t* poff;     // [G+1] pixel offset of each group in the buffer
    const int32_t* toff256;  // [G+1] cumulative 256-pixel tile counts
    const int32_t* loff;     // [G+1] cumulative image (line) counts
    int ntiles256;
    const int32_t* toff2d;   // [G+1] cumulative TH x TW patch counts (conv3x3_ragged), TH = 128 / tw
    int ntiles2d, tw;
    // the same with the patches tiling the whole group's strip of images (flat column = img * Wp + x; Wp = W, or W
    // rounded up to even in the *_flat2 table of a layer whose epilogue pools horizontally)
    const int32_t* toff2d_flat;
    const int32_t* toff2d_flat2;
    int ntiles2d_flat, ntiles2d_flat2;
    // the 4 x 32 tables whatever tw says: the row-owning form of conv3x3_ragged (an engine's "conv_rows") tiles no other shape
    const int32_t* toff2d_32;
    const int32_t* toff2d_flat_32;
    const int32_t* toff2d_flat2_32;
    int ntiles2d_32, ntiles2d_flat_32, ntiles2d_flat2_32;   // 0 when H % 4 != 0
    int64_t max_tile_px32_;  // max_tile_px_ for 32-column flat tiles (host)
    const int32_t* toff2d_gap;   // 8 x 16 patches over the strip with >= 1 empty column between images (conv12_fused_ragged)
    int ntiles2d_gap;
    int64_t max_tile_px_;    // most pixels in the images one flat tile touches (host)
    int min_w;               // narrowest image at this layer (host)
    int64_t pixels;          // total pixels (host)
    int max_w;               // widest image at this layer (host)
};
void conv1_relu_pool_ragged(const float* x, const RaggedView& in, const float* wt, const float* bias, int cout,
                            float* y, const RaggedView& out, hipStream_t s);
void pool_ragged(const float* x, const RaggedView& in, int c, int kh, int kw, bool avg, float* y, const RaggedView& out,
                 hipStream_t s);
void to_seq_packed_ragged(const float* x, const RaggedView& in, int c, const int32_t* d_pos, const int32_t* d_off,
                          float* y, hipStream_t s);
// AvgPool (in.H, 1) + the sequence packing in one pass (`in`: geometry before the pool, `seq`: after it, height 1)
void avgpool_to_seq_ragged(const float* x, const RaggedView& in, const RaggedView& seq, int c, const int32_t* d_pos,
                           const int32_t* d_off, float* y, hipStream_t s);
// conv1 (Cin = 1) + ReLU + pool 2x2 + conv2 + ReLU + pool 2x2 in one launch; false = not this shape (run the two ops)
// w2split: conv2's weights cut into bf16 terms (conv12_split_weights) or null; used when the calling engine's numerics are not exact
bool conv12_fused_ragged(const float* x, const RaggedView& in0, const RaggedView& mid, const float* w1, const float* b1,
                         int c1, const float* w2, const float* b2, int c2, float* y, const RaggedView& out, hipStream_t s,
                         const uint16_t* w2split = nullptr);
void conv12_split_weights(const float* w2_host /* [288][64] */, std::vector<uint16_t>* out);   // host
// returns false if the shape is not supported (caller falls back to the per-group path)
// wsplit: the weights cut into bf16 terms (split_mfma.hpp split_weights) or null; used when the calling engine's numerics are not exact
// skip_exact: dropping the MFMAs of out-of-image tap rows leaves every bit as it is (conv_rows.hpp; "conv_rows" = 2 then does)
bool conv3x3_ragged(const float* x, const RaggedView& rv, int cin, const float* wt, const float* bias, int cout, int relu,
                    int ph, int pw, float* y, const RaggedView& out, hipStream_t s, const uint16_t* wsplit = nullptr,
                    bool skip_exact = false);
void split_weights(const float* w_host, int K, int N, int ldw, std::vector<uint16_t>* out);   // host; N % 128 == 0, K % 16 == 0 (split_mfma.hpp)

// ---- kernels_lines.hip ----------------------------------------------------
struct LineDesc {      // one text line to crop (recognition.rs:91-126)
    int32_t page;      // index into page pointer table
    int32_t poly_off;  // first vertex in the packed polygon array
    int32_t poly_n;    // vertex count
    int32_t top, left, bh, bw;  // polygon bounding rect (exclusive bottom/right)
    int32_t resized_w;
    int32_t out_w;     // padded width of this line's batch (its width group)
    int64_t out_off;   // float offset of this line's [out_h, out_w] image in the output buffer
};
// Fill + gather + bilinear resize + right-pad with -0.5; every line writes its own
// [out_h, out_w] image at d_out + out_off (lines of different width groups in one launch).
void crop_lines(const float* const* d_pages, const int32_t* d_page_hw /*[pages][2]*/, const LineDesc* d_lines,
                const int32_t* d_poly /*(y,x) pairs*/, int n_lines, int out_h, float* d_out, hipStream_t s);

// ---- kernels_rectify.hip -----------------------------------
struct RectLineDesc {   // one text line to crop along its own axis: LineDesc's sibling
    int32_t page;       // index into page pointer table
    int32_t mode;       // 0: sample through the map; 1: an empty line, all -0.5
    int32_t range_off;  // first word in the packed range array (4 ints per word: c0, c1, r0, r1; c0 > c1 covers nothing)
    int32_t range_n;    // word count
    int32_t resized_w;
    int32_t out_w;      // padded width of this line's batch (its width group); even
    int64_t out_off;    // float offset of this line's [out_h, out_w] image in the output buffer; even
    float x0, ax, bx, y0, ay, by;   // X = (x0 + ax * (ox + 0.5)) + bx * (oy + 0.5), Y likewise
};
// Affine gather + bilinear taps + per-column row mask + right-pad with -0.5; every line writes its own [out_h, out_w]
// image at d_out + out_off, as crop_lines does.  max_out_w: the widest out_w among the lines.  d_ranges: 16-byte aligned.
void rectify_lines(const float* const* d_pages, const int32_t* d_page_hw /*[pages][2]*/, const RectLineDesc* d_lines,
                   const int32_t* d_ranges, int n_lines, int max_out_w, int out_h, float* d_out, hipStream_t s);

// ---- kernels_rotate.hip ------------------------------------
struct RotateDesc {      // one page to turn: dst = np.rot90(src, k)
    const uint32_t* src; // [h, w] pixels as 32-bit words
    uint32_t* dst;       // [h, w] for k even, [w, h] for k odd; never overlaps src
    int32_t h, w;        // of the source
    int32_t k;           // quarter turns counter-clockwise, 0 .. 3
    int32_t block0;      // first block of this page: the sum of rotate_tiles() of the pages before it
    int32_t vec;         // k even only: w % 4 == 0 and both buffers 16-byte aligned, so 16-byte accesses are safe
    int32_t pad_;
};
int64_t rotate_tiles(int h, int w);   // blocks a page of this size takes (host)
// Pages of any mix of sizes and turns in one launch; total_tiles = the sum of rotate_tiles() over the pages.
void rotate_pages(const RotateDesc* d_descs, int n_pages, int total_tiles, hipStream_t s);

// ---- kernels_resample.hip ----------------------------------
struct ResampleDesc {    // one page to resample: dst [dh, dw] from src [sh, sw]
    const float* src;
    float* dst;          // never overlaps src
    int32_t sh, sw, dh, dw;   // each 1 .. 65535
    int32_t area;        // 1: the area filter (dh <= sh and dw <= sw), 0: bilinear
    int32_t block0;      // first block of this page: the sum of resample_blocks() of the pages before it
    uint32_t py, qy;     // area only: sh / gcd(sh, dh), dh / gcd(sh, dh)
    uint32_t px, qx;     // likewise along x
};
int64_t resample_blocks(int dh, int dw);   // blocks an output of this size takes (host)
// Pages of any mix of sizes and filters in one launch; total_blocks = the sum of resample_blocks() over the pages.
void resample_pages(const ResampleDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// ---- kernels_normalize.hip ---------------------------------
struct NormInfo {        // what a page's normalisation found: the layout of ocrs_normalize_info
    int32_t dark;        // 1: read as light text on a dark page and inverted
    int32_t white;       // Wg: the white bin of the page's effective histogram; -1: no pixel counted
    int32_t lo, hi;      // the bins of u that levels stretched between; -1, -1 with levels off
    int64_t vote;        // the polarity vote; 0 unless polarity is auto
    uint64_t counted;    // pixels that are not NaN
};
struct NormState {       // per page, zeroed before the first pass
    unsigned long long hist_v[256];   // page histogram of clamp(v + 0.5) (pass 1)
    unsigned long long hist_u[256];   // page histogram of u (pass 3)
    long long vote;                   // pass 1
    NormInfo info;                    // passes 2 and 4
};
struct NormDesc {        // one page to normalise: dst [h, w] from src [h, w]
    const float* src;
    float* dst;          // never overlaps src
    NormState* state;
    uint32_t* tiles;     // [th, tw] what pass 1 keeps of a tile's histogram: pct(3,4) as it is | pct(3,4) read mirrored << 8 |
                         // (the tile counted a pixel) << 16
    uint8_t* grid;       // [th, tw] level bins (pass 2)
    int32_t h, w;        // each 1 .. 65535
    int32_t tshift;      // log2 of the tile size, 4 .. 8
    int32_t th, tw;      // ceil(h / T), ceil(w / T)
    int32_t block0;      // first block of this page: the sum of th * tw of the pages before it
    int32_t polarity;    // 0 auto, 1 keep, 2 invert
    int32_t flatten, levels;
    int32_t vec;         // w % 4 == 0 and both buffers 16-byte aligned, so 16-byte accesses are safe
};
// Pages of any mix of sizes and parameters, five launches on `s`; total_blocks = the sum of th * tw over the pages.  The
// states must be zero when the first launch starts.  d_info[n_pages] receives each page's NormInfo.
void normalize_pages(const NormDesc* d_descs, int n_pages, int total_blocks, NormInfo* d_info, hipStream_t s);

// ---- kernels_deskew.hip ------------------------------------
struct SkewDesc {        // one page whose skew profiles are taken
    const float* src;    // [h, w]
    uint32_t* prof;      // [n_angles, nb] the page's profiles; zero when the launch starts
    int32_t h, w;        // each 1 .. 4096
    int32_t nb;          // h + w: dwords per profile
    int32_t block0;      // first block of this page: the sum of skew_tiles() of the pages before it
};
int64_t skew_tiles(int h, int w);   // blocks a page of this size takes (host)
// Pages of any mix of sizes, two launches on `s`; total_tiles = the sum of skew_tiles() over the pages.  d_sc_table:
// int32 [n_angles, 2] (S, C), each within +-65536.  d_scores [n_pages, n_angles].  n_pages <= 65535.
void skew_scores(const SkewDesc* d_descs, int n_pages, int total_tiles, const int32_t* d_sc_table, int n_angles,
                 unsigned long long* d_scores, hipStream_t s);
struct WarpDesc {        // one page to warp: dst [dh, dw] from src [sh, sw]
    const float* src;
    float* dst;          // never overlaps src
    int32_t sh, sw, dh, dw;   // each 1 .. 65535
    int32_t block0;      // first block of this page: the sum of warp_blocks() of the pages before it
    int32_t vec;         // dw % 4 == 0 and dst 16-byte aligned, so 16-byte stores are safe
    float m[6];          // X = (m0 + m1 fx) + m2 fy, Y = (m3 + m4 fx) + m5 fy
    float fill;          // a tap outside the page
    int32_t pad_;
};
int64_t warp_blocks(int dh, int dw);   // blocks an output of this size takes (host)
// Pages of any mix of sizes and maps in one launch; total_blocks = the sum of warp_blocks() over the pages.
void warp_pages(const WarpDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// ---- kernels_perspective.hip -------------------------------
struct EdgeDesc {        // one page whose edge peaks are taken
    const float* src;    // [h, w]
    uint32_t* prof;      // [2 families, 2 signs, n_angles, nb] the page's edge counts; zero when the launch starts
    unsigned long long* peaks;   // [2 families, 2 signs, n_angles, 16]
    int32_t h, w;        // each 1 .. 4096
    int32_t nb;          // h + w: dwords per profile
    int32_t block0;      // first block of this page: the sum of edge_tiles() of the pages before it
};
int64_t edge_tiles(int h, int w);   // blocks a page of this size takes (host)
// Pages of any mix of sizes, two launches on `s`; total_tiles = the sum of edge_tiles() over the pages.  d_sc_table: int32
// [n_angles, 2] (S, C), each within +-65536.  min_step 1 .. 256.  n_pages <= 65535 (the peak kernel's grid.y), n_angles <= 65535.
void edge_peaks(const EdgeDesc* d_descs, int n_pages, int total_tiles, const int32_t* d_sc_table, int n_angles, int min_step, hipStream_t s);
struct ProjDesc {        // one page to project: dst [dh, dw] from src [sh, sw]
    const float* src;
    float* dst;          // never overlaps src
    int32_t sh, sw, dh, dw;   // each 1 .. 65535
    int32_t block0;      // first block of this page: the sum of project_blocks() of the pages before it
    int32_t vec;         // dw % 4 == 0 and dst 16-byte aligned, so 16-byte stores are safe
    float m[8];          // X = ((m0 + m1 fx) + m2 fy) / dn, Y = ((m3 + m4 fx) + m5 fy) / dn, dn = (1 + m6 fx) + m7 fy
    float fill;          // a tap outside the page, and a pixel whose dn is not finite and positive
    int32_t pad_;
};
int64_t project_blocks(int dh, int dw);   // blocks an output of this size takes (host)
// Pages of any mix of sizes and maps in one launch; total_blocks = the sum of project_blocks() over the pages.
void project_pages(const ProjDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// ---- kernels_rules.hip -------------------------------------
struct RulesInfo {       // what a page's rule removal found: the layout of ocrs_rules_info
    int32_t paper_bin;   // the bin the fill was taken from; -1: the fill was given
    float fill;          // what the removed pixels were overwritten with
    uint64_t ink;        // pixels under the threshold
    uint64_t counted;    // pixels that are neither ink nor NaN
    uint64_t h_removed, v_removed;   // |Dh|, |Dv|
    uint64_t overwritten;            // |D|
    uint64_t kept;                   // |Kh u Kv|
};
// The bit masks of a page, 64 pixels to a word.  Row-major masks: [h, ww] words, bit c of word (y, j) = pixel (y, 64 j + c).
// Transposed masks: [w, hw] words, bit r of word (x, j) = pixel (64 j + r, x).  Bits past the page's edge are zero.
enum RulesMask {
    RM_INK = 0, RM_CH, RM_CV, RM_RV, RM_DV, RM_MV, RM_ROW_MAJOR,                      // row-major
    RM_INK_T = 0, RM_CV_T, RM_CH_T, RM_RH_T, RM_DH_T, RM_MH_T, RM_TRANSPOSED          // transposed
};
constexpr int RULES_COUNTS = 16;
struct RulesDesc {       // one page whose rules are removed: dst [h, w] from src [h, w]
    const float* src;
    float* dst;          // never overlaps src
    unsigned long long* masks;   // rules_mask_words(h, w) words: RM_ROW_MAJOR masks of h * ww, then RM_TRANSPOSED of w * hw
    unsigned long long* hist;    // [256] the histogram of the pixels that are neither ink nor NaN; zero when the first launch starts
    unsigned long long* counts;  // [hw * ww, RULES_COUNTS] what each block counted
    RulesInfo* info;
    uint8_t* mask_out;   // [h, w] the mask of include/ocrs_amd.h, or null
    int32_t h, w;        // each 1 .. 65535
    int32_t ww, hw;      // ceil(w / 64), ceil(h / 64)
    int32_t block0;      // first block of this page: the sum of hw * ww of the pages before it
    int32_t min_length, max_thickness, margin;   // 2 .. 65535, 1 .. 64, 0 .. 8
    float threshold;
    float paper;         // NaN: measured
    int32_t vec;         // w % 4 == 0 and both buffers 16-byte aligned, so 16-byte accesses are safe
    int32_t pad_;
};
int64_t rules_tiles(int h, int w);        // blocks a page of this size takes (host)
size_t rules_mask_words(int h, int w);    // 64-bit words of RulesDesc::masks (host)
// Pages of any mix of sizes and parameters, eight launches on `s`; total_blocks = the sum of rules_tiles() over the pages.
void remove_rules_pages(const RulesDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// ---- kernels_speckle.hip -----------------------------------
struct SpeckleInfo {     // what a page's despeckling found: the layout of ocrs_speckle_info
    int32_t paper_bin;   // the bin the specks' fill was taken from; -1: the fill was given
    int32_t ink_bin;     // the bin the holes' fill was taken from; -1: the fill was given
    float paper_fill;    // what the specks were overwritten with
    float ink_fill;      // what the holes were overwritten with
    uint64_t ink;        // pixels under the threshold
    uint64_t counted;    // pixels that are neither ink nor NaN
    uint64_t specks, kept;               // components removed; candidates kept for being near big ink
    uint64_t speck_pixels, kept_pixels;  // their pixels
    uint64_t holes, hole_pixels;         // paper components filled, and their pixels
};
constexpr int SPECKLE_COUNTS = 32;   // 64-bit words of a block's record: [wave][8]
constexpr int SPECKLE_MAX_AREA = 4096, SPECKLE_MAX_NEAR = 16;
struct SpeckleDesc {     // one page that is despeckled: dst [h, w] from src [h, w]
    const float* src;
    float* dst;          // never overlaps src
    unsigned long long* masks;   // 3 row-major bit masks of h * ww words (64 pixels a word, bits past the edge zero): ink, big, near
    int32_t* labels;     // [h * w] the union-find forest over page-local pixel indices, both classes
    uint32_t* area;      // [h * w] at a root: the pixels of its component
    uint8_t* near_flag;  // [h * w] at a root: 1 when a pixel of this candidate component lies within keep_near of big ink
    unsigned long long* hist;    // [2][256] paper pixels (neither ink nor NaN), ink pixels; zero when the first launch starts
    unsigned long long* counts;  // [hw * ww, SPECKLE_COUNTS] what each block counted
    SpeckleInfo* info;
    uint8_t* mask_out;   // [h, w] the mask of include/ocrs_amd.h, or null
    int32_t h, w;        // each 1 .. 65535, h * w < 2^31
    int32_t ww, hw;      // ceil(w / 64), ceil(h / 64)
    int32_t block0;      // first block of this page: the sum of hw * ww of the pages before it
    int32_t max_area, max_hole, keep_near;   // 0 .. 4096, 0 .. 4096, 0 .. 16
    float threshold;
    float paper, ink_level;   // NaN: measured
    int32_t vec;         // w % 4 == 0 and both buffers 16-byte aligned, so 16-byte accesses are safe
};
int64_t speckle_tiles(int h, int w);        // blocks a page of this size takes (host)
size_t speckle_mask_words(int h, int w);    // 64-bit words of SpeckleDesc::masks (host)
// Pages of any mix of sizes and parameters, eight launches on `s`; total_blocks = the sum of speckle_tiles() over the pages.
void despeckle_pages(const SpeckleDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// ---- kernels_binarize.hip ---------------------------------
struct BinInfo {         // what a page's binarisation counted: the layout of ocrs_binarize_info
    uint64_t counted;    // pixels that are not NaN
    uint64_t ink;        // counted pixels the local rule calls ink
    float ink_fill;      // what ink was written as (keep_ink: not written)
    float paper_fill;    // what every other counted pixel was written as
};
constexpr int BIN_COUNTS = 8;        // 64-bit words of a block's record: [wave][2]
constexpr int BIN_MAX_RADIUS = 127, BIN_MAX_KQ = 256;
constexpr int BIN_STRIP = 256;       // columns of a block of the vertical pass: a lane per column
constexpr int BIN_ROWS = 4;          // rows of a block of the horizontal pass: a wave per row
struct BinDesc {         // one page that is binarised: dst [h, w] from src [h, w]
    const float* src;
    float* dst;          // never overlaps src
    uint32_t* sums;      // [h * w][2] per pixel, over [x - r, x + r] of its row: n << 16 | S, and Q
    unsigned long long* counts;  // [blocks of the vertical pass, BIN_COUNTS] what each block counted
    BinInfo* info;
    uint8_t* mask_out;   // [h, w] the mask of include/ocrs_amd.h, or null
    int32_t h, w;        // each 1 .. 65535, h * w < 2^31
    int32_t block0;      // first block of this page in the vertical pass: the sum of strips * segs of the pages before it
    int32_t row_block0;  // first block of this page in the horizontal pass: the sum of ceil(h / BIN_ROWS) before it
    int32_t strips, segs;   // ceil(w / BIN_STRIP), ceil(h / seg_rows)
    int32_t seg_rows;    // rows of a block of the vertical pass (bin_seg_rows)
    int32_t radius, kq;  // 1 .. 127, 0 .. 256
    int32_t keep_ink;    // 0 / 1
    uint32_t ink_bits, paper_bits;   // the fills as 32-bit words, defaults resolved
};
int bin_seg_rows(int h, int w, int radius);       // rows of a block of the vertical pass (host)
int64_t bin_col_blocks(int h, int w, int radius); // blocks a page takes in the vertical pass (host)
int64_t bin_row_blocks(int h);                    // blocks a page takes in the horizontal pass (host)
// Pages of any mix of sizes and parameters, three launches on `s`; row_blocks and col_blocks are the sums over the pages.
void binarize_pages(const BinDesc* d_descs, int n_pages, int row_blocks, int col_blocks, hipStream_t s);

// ---- kernels_morph.hip ------------------------------------
struct MorphInfo {       // what a page's stroke repair counted: the layout of ocrs_morph_info
    uint64_t counted;    // pixels that are not NaN
    uint64_t changed;    // counted pixels whose 32-bit word changed
    uint64_t ink_before; // counted pixels under 0.0f on the source
    uint64_t ink_after;  // counted pixels under 0.0f on the result
};
constexpr int MORPH_COUNTS = 4;       // 64-bit words of a block's record: the four counts of MorphInfo
constexpr int MORPH_MAX_RADIUS = 63;
constexpr int MORPH_OPS = 4;          // thicken (lo), thin (hi), close (lo, hi), open (hi, lo): OCRS_MORPH_*
constexpr int MORPH_STRIP = 64;       // columns of a block of the vertical pass: a lane per column, one wave
constexpr int MORPH_ROWS = 4;         // rows of a block of the horizontal pass: a wave per row
constexpr int MORPH_SEG = 256;        // columns of a block of the horizontal pass
struct MorphDesc {       // one page that is repaired: dst [h, w] from src [h, w], in one or two stages
    const float* src;
    float* dst;          // never overlaps src
    float* mid;          // [h, w] the page between the stages of close and open; null for thicken and thin
    uint32_t* keys;      // [h, w] the row extrema of the stage at hand as ordered keys (NaN: the empty key), at every pixel
    unsigned long long* counts;  // [strips * segs, MORPH_COUNTS] what each block of the last vertical pass counted
    MorphInfo* info;
    uint8_t* mask_out;   // [h, w] the mask of include/ocrs_amd.h, or null
    int32_t h, w;        // each 1 .. 65535, h * w < 2^31
    int32_t block0;      // first block of this page in the vertical pass of stage 1: the sum of strips * segs before it
    int32_t row_block0;  // ... in the horizontal pass of stage 1: the sum of row_blocks before it
    int32_t block0_2;    // ... in the vertical pass of stage 2: pages of one stage take no blocks there
    int32_t row_block0_2;   // ... in the horizontal pass of stage 2
    int32_t strips, segs;   // ceil(w / MORPH_STRIP), ceil(h / seg_rows)
    int32_t seg_rows;    // rows of a block of the vertical pass (morph_seg_rows): a multiple of 2 ry + 1
    int32_t row_segs;    // ceil(w / MORPH_SEG)
    int32_t rx, ry;      // 0 .. 63, not both 0
    int32_t stages;      // 1 or 2
    uint32_t flip[2];    // per stage: 0 for lo, ~0 for hi; the stage takes the least of key ^ flip
};
int morph_seg_rows(int h, int w, int ry);         // rows of a block of the vertical pass (host)
int64_t morph_col_blocks(int h, int w, int ry);   // blocks a page takes in a vertical pass (host)
int64_t morph_row_blocks(int h, int w);           // blocks a page takes in a horizontal pass (host)
// Pages of any mix of sizes, ops and radii; at most five launches on `s`.  row_blocks[s] and col_blocks[s] are the sums over
// the pages of stage s + 1; a page of one stage adds nothing to those of stage 2.  max_ry: the largest ry of the batch, by
// which the vertical pass sizes its LDS.
void morph_pages(const MorphDesc* d_descs, int n_pages, const int row_blocks[2], const int col_blocks[2], int max_ry, hipStream_t s);

// ---- kernels_rank.hip -------------------------------------
struct RankInfo {        // what a page's grain removal counted: the layout of ocrs_rank_info
    uint64_t counted;    // pixels that are not NaN
    uint64_t changed;    // counted pixels whose 32-bit word changed
    uint64_t ink_before; // counted pixels under 0.0f on the source
    uint64_t ink_after;  // counted pixels under 0.0f on the result
    uint64_t spared;     // counted pixels that kept their word by the sparing rule
};
constexpr int RANK_COUNTS = 5;        // 64-bit words of a block's record: the five counts of RankInfo
constexpr int RANK_MAX_RADIUS = 7;
constexpr int RANK_TILE_W = 64;       // columns of a block's tile: a lane per column
constexpr int RANK_TILE_H = 16;       // rows of a block's tile: four waves, four rows each
struct RankDesc {        // one page that is filtered: dst [h, w] from src [h, w]
    const float* src;
    float* dst;          // never overlaps src
    unsigned long long* counts;  // [tiles_y * tiles_x, RANK_COUNTS] what each block counted
    RankInfo* info;
    uint8_t* mask_out;   // [h, w] the mask of include/ocrs_amd.h, or null
    int32_t h, w;        // each 1 .. 65535, h * w < 2^31
    int32_t block0;      // the sum of tiles_y * tiles_x over the pages before it: where the page's records lie in the batch's
    int32_t reg_block0;  // the page's first block in the launch of the register classes: pages of class 2 take no blocks there
    int32_t lds_block0;  // ... in the launch of class 2: pages of the register classes take no blocks there
    int32_t tiles_x, tiles_y;   // ceil(w / RANK_TILE_W), ceil(h / RANK_TILE_H)
    int32_t rx, ry;      // 0 .. 7, not both 0
    int32_t percent;     // 0 .. 100
    int32_t tail;        // 0 .. 50; 0: no pixel is spared
    int32_t cls;         // rank_class(rx, ry): how the kernel holds the window
};
int64_t rank_blocks(int h, int w);   // blocks a page of this size takes (host)
int rank_class(int rx, int ry);      // 0: a 3 x 3 window in registers, 1: 5 x 5 in registers, 2: walked in LDS (host)
// Pages of any mix of sizes and parameters, at most three launches on `s`; reg_blocks and lds_blocks are the sums of
// rank_blocks() over the pages of classes 0 and 1, and of class 2.
void rank_pages(const RankDesc* d_descs, int n_pages, int reg_blocks, int lds_blocks, hipStream_t s);

// ---- kernels_frame.hip ------------------------------------
struct FrameInfo {       // what a page's frame cleanup found: the layout of ocrs_frame_info
    int32_t paper_bin;   // the bin the fill was taken from; -1: the fill was given
    float paper_fill;    // what the removed ink was overwritten with
    uint64_t ink;        // pixels under the threshold
    uint64_t counted;    // pixels that are neither ink nor NaN
    uint64_t ring_ink;   // |R|: ink inside the ring
    uint64_t removed, removed_pixels;   // touching components of area >= min_area, and their pixels
    uint64_t kept, kept_pixels;         // touching components of area < min_area, and their pixels
};
constexpr int FRAME_COUNTS = 32;   // 64-bit words of a block's record: [wave][8]
struct FrameDesc {       // one page whose frame is cleaned: dst [h, w] from src [h, w]
    const float* src;
    float* dst;          // never overlaps src
    unsigned long long* rmask;   // the row-major bit mask of R = ink in the ring: h * ww words (64 pixels a word, bits past the edge zero)
    int32_t* labels;     // [h * w] the union-find forest over the pixels of R (the other entries are never written or read)
    uint32_t* area;      // [h * w] at a root: the pixels of its component
    uint8_t* seed_flag;  // [h * w] at a root: 1 when a pixel of its component lies on an enabled side
    unsigned long long* hist;    // [256] paper pixels (neither ink nor NaN); zero when the first launch starts
    unsigned long long* counts;  // [hw * ww, FRAME_COUNTS] what each block counted
    FrameInfo* info;
    uint8_t* mask_out;   // [h, w] the mask of include/ocrs_amd.h, or null
    int32_t h, w;        // each 1 .. 65535, h * w < 2^31
    int32_t ww, hw;      // ceil(w / 64), ceil(h / 64)
    int32_t block0;      // the page's first block (one per 64 x 64 tile): the sum of hw * ww over the pages before it
    int32_t depth, sides, min_area;
    float threshold;
    float paper;         // NaN: measured
    int32_t vec;         // w % 4 == 0 and the buffers 16-byte aligned, so 16-byte accesses are safe
};
int64_t frame_tiles(int h, int w);   // blocks a page of this size takes (host)
// Pages of any mix of sizes and parameters, six launches on `s`; total_blocks = the sum of frame_tiles() over the pages.
void clean_frame_pages(const FrameDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);
// cols[w] and rows[h] (either may be null; zero when the launch starts) += the pixels of src [h, w] under `threshold`; one launch
void ink_profiles(const float* src, int h, int w, float threshold, uint32_t* cols, uint32_t* rows, hipStream_t s);
struct CropDesc {        // one rectangle cut out of a page: dst [oh, ow] = src [y0 .. y0 + oh, x0 .. x0 + ow), `fill` outside src
    const uint32_t* src;
    uint32_t* dst;
    int32_t h, w;        // of src
    int32_t oh, ow;      // each 1 .. 65535
    int32_t x0, y0;      // any int32
    uint32_t fill;       // the 32-bit word of a pixel outside src
    int32_t block0;      // the page's first block (one per 64 x 64 tile of dst)
    int32_t vec;         // ow % 4 == 0 and dst 16-byte aligned: 16-byte stores
};
void crop_pages(const CropDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// ---- kernels_measure.hip ----------------------------------
constexpr int MEASURE_BINS = 256;        // a length, height or width L is counted at min(L, 255)
constexpr int MEASURE_MAX_MIN_AREA = 65535;
struct MeasureInfo {     // what a page's measurement counted: the layout of ocrs_measure_info
    uint64_t ink;        // pixels under the threshold
    uint32_t components; // 8-connected components of ink
    uint32_t counted;    // those of area >= min_area
    uint32_t run_h[MEASURE_BINS], run_v[MEASURE_BINS];     // maximal horizontal / vertical runs of ink by length
    uint32_t comp_h[MEASURE_BINS], comp_w[MEASURE_BINS];   // counted components by the height / width of their box
    uint64_t area_by_h[MEASURE_BINS];                      // their summed areas, by the height
};
struct MeasureDesc {     // one page that is measured; nothing is made of it
    const float* src;    // [h, w]
    unsigned long long* mask;    // the row-major ink bit mask of h * ww words (64 pixels a word, bits past the edge zero)
    int32_t* labels;     // [h * w] the union-find forest over page-local pixel indices; written and read on ink alone
    uint32_t* area;      // [h * w] at a root: the pixels of its component.  This and the three box words are written at
    uint32_t* x0;        // [h * w] the heads of the in-word runs of ink alone: a root is one of them.  The least x,
    uint32_t* x1;        // [h * w] the largest x
    uint32_t* y1;        // [h * w] and the largest y of its component; the least y is that of the root itself
    MeasureInfo* info;   // zero when the first launch starts; every launch adds to it
    int32_t h, w;        // each 1 .. 65535, h * w < 2^31
    int32_t ww;          // ceil(w / 64)
    int32_t block0;      // first block of this page: the sum of measure_tiles() of the pages before it
    int32_t min_area;    // 0 .. 65535
    float threshold;
};
int64_t measure_tiles(int h, int w);        // blocks a page of this size takes (host)
size_t measure_mask_words(int h, int w);    // 64-bit words of MeasureDesc::mask (host)
// Pages of any mix of sizes and parameters, five launches on `s`; total_blocks = the sum of measure_tiles() over the pages.
void measure_pages(const MeasureDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// ---- kernels_reverse.hip ----------------------------------
struct ReverseInfo {     // what a page's reverse-video repair found: the layout of ocrs_reverse_info
    uint64_t ink;            // pixels under the threshold
    uint64_t components;     // 8-connected components of ink
    uint64_t candidates;     // those large and solid enough to be a panel
    uint64_t panels;         // candidates that enclose at least min_holes counting holes
    uint64_t panel_pixels;   // their pixels
    uint64_t holes;          // counting holes of panels
    uint64_t hole_pixels;    // their pixels
    uint64_t skipped_holes;  // holes of panels larger than max_hole: left as they are
    uint64_t inverted;       // panel_pixels + hole_pixels
};
constexpr int REVERSE_COUNTS = 32;   // 64-bit words of a block's record: [wave][8]
constexpr int REVERSE_MAX_SIDE = 65535;
constexpr int REVERSE_WORKSPACE_PER_PIXEL = 20;   // bytes: labels, area and three box words; and two bits of masks
struct ReverseDesc {     // one page that is repaired: dst [h, w] from src [h, w]
    const float* src;
    float* dst;          // never overlaps src
    unsigned long long* masks;   // 2 row-major bit masks of h * ww words (64 pixels a word, bits past the edge zero): ink, M
    int32_t* labels;     // [h * w] two union-find forests over page-local pixel indices that never unite: the ink's (8-connected;
                         // from pass 4 on kept on M alone) and, from pass 4 on, that of everything outside M (4-connected)
    uint32_t* area;      // [h * w] at a root: the pixels of its component (ink until pass 4, outside M from pass 5 on)
    uint32_t* x0;        // [h * w] at an ink root: the least x of its component; from pass 5 on, at a root outside M: 1 when
                         // its component touches the page's edge
    uint32_t* x1;        // [h * w] at an ink root: the largest x; from pass 5 on, at a root of M: its counting holes
    uint32_t* y1;        // [h * w] at an ink root: the largest y; the least y is that of the root itself
    unsigned long long* counts;  // [hw * ww, REVERSE_COUNTS] what each block counted
    ReverseInfo* info;
    uint8_t* mask_out;   // [h, w] the mask of include/ocrs_amd.h, or null
    int32_t h, w;        // each 1 .. 65535, h * w < 2^31
    int32_t ww, hw;      // ceil(w / 64), ceil(h / 64)
    int32_t block0;      // first block of this page: the sum of hw * ww of the pages before it
    int32_t min_height, min_width;   // 1 .. 65535
    int32_t fill_q8;     // floor(256 min_fill + 0.5): 0 .. 256
    int32_t min_holes, max_hole;     // >= 0; max_hole 0: no limit
    float threshold;
    int32_t vec;         // w % 4 == 0 and the buffers 16-byte aligned, so 16-byte accesses are safe
};
int64_t reverse_tiles(int h, int w);        // blocks a page of this size takes (host)
size_t reverse_mask_words(int h, int w);    // 64-bit words of ReverseDesc::masks (host)
int reverse_fill_q8(float min_fill);        // (host)
// Pages of any mix of sizes and parameters, nine launches on `s`; total_blocks = the sum of reverse_tiles() over the pages.
void unreverse_pages(const ReverseDesc* d_descs, int n_pages, int total_blocks, hipStream_t s);

// kernels_peaks.hip
void measure_peaks(double* mfma_tflops, double* copy_gbps);


// kernels_jpeg.hip — the GPU half of the JPEG hand-off (jpeg.hpp)
size_t jpeg_sample_bytes(const jpeg::Coefficients& c);
void jpeg_decode(const jpeg::Coefficients& c, const uint64_t* d_mask, const uint32_t* d_offset, const int16_t* d_values,
                 const uint16_t* d_quant, uint8_t* d_samples, uint8_t* d_rgb, hipStream_t s);

}  // namespace k
}  // namespace ocrs
