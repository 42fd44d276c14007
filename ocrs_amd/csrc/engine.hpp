// OcrEngine (ocrs/src/lib.rs:111-301) on MI355X: the grey page stays in HBM
// between prepare_input / detect_words / recognize_text.
#pragma once
#include <string>
#include <vector>

#include <memory>

#include "coalesce.hpp"
#include "common.hpp"
#include "geometry.hpp"
#include "model.hpp"

struct ocrs_page {  // OcrInput (lib.rs:125-128)
    ocrs::DevBuf grey;  // [h, w] fp32 in [-0.5, 0.5]; on the device of the engine that prepared it
    int h = 0, w = 0;
    // the host pixels an engine GROUP prepared this page from (group.cpp: key of the replay mode's recorded results); else null
    const void* source = nullptr;
    int device() const { return grey.device(); }
};

namespace ocrs {

struct CtcStep { uint32_t label, pos; };

// ctc_beam.cpp — rten decode_beam (recognition.rs:512-514).  score (optional): the best beam's lse(pb, pnb).
std::vector<CtcStep> ctc_beam_search(const float* logp, int T, int C, int row_stride, uint32_t width, double* score = nullptr);
// the same function written as the algorithm is usually stated (trie + candidate map); tests compare the two
std::vector<CtcStep> ctc_beam_search_reference(const float* logp, int T, int C, int row_stride, uint32_t width,
                                               double* score = nullptr);

// The host form of recognition confidence (RecResult below) for one line whose log-probs are on the host: row t at
// logp + t * row_stride, labels flagged in `excluded` ([C] or null) read as -inf.  beam_score given: the line score is that
// value (beam search); null: the greedy path's.  The GPU kernels compute the same bits (ctc_collapse_scored_packed, ctc_beam_packed).
void score_line(const float* logp, int T, int C, size_t row_stride, const uint8_t* excluded, const std::vector<CtcStep>& steps,
                const double* beam_score, std::vector<float>* step_logp, double* line_score);

struct TextChar {  // text_items.rs:48-54
    uint32_t ch;
    geom::Rect rect;
};

// Rectified line crops: a line's own frame from its word rects (cx, cy, upx, upy, w, h), on the host in
// double — the axis through the word centres, the extents of the words' corners along it and across it, the output width,
// the six float32 coefficients of the sampling map and every word's column / row range of the mask.
struct LineFrame {
    bool empty = true;                       // degenerate: the crop is all -0.5 and the line has no char boxes
    double ax = 0.0, ay = 0.0;               // axis a; the normal is (-ay, ax)
    double s_min = 0.0, s_max = 0.0, t_min = 0.0, t_max = 0.0;
    uint32_t rw = 0;
    float coef[6] = {0, 0, 0, 0, 0, 0};      // x0, ax, bx, y0, ay, by
    std::vector<int32_t> ranges;             // [n][4]: c0, c1, r0, r1 (c0 > c1: the word covers nothing)
};
LineFrame line_frame(const float* words6, size_t n_words, int32_t rec_height);
// the page boxes of a rectified line's chars from its CTC step positions: (step index, box) of every char that is kept
std::vector<std::pair<size_t, geom::Rect>> rectified_char_boxes(const LineFrame& f, uint32_t group_width, uint32_t ctc_input_len,
                                                                const uint32_t* pos, size_t n_steps);

struct RecLine {  // TextRecLine (recognition.rs:80-89) + owning page
    size_t page = 0;
    size_t index = 0;                    // line index in the caller's order
    std::vector<geom::PointI> polygon;   // line_polygon (recognition.rs:29-55)
    geom::Rect bounds{0, 0, 0, 0};       // Polygon::bounding_rect
    uint32_t resized_width = 0;
    uint32_t group_width = 0;
    bool rectified = false;              // cropped along its own axis (frame) instead of through polygon / bounds
    LineFrame frame;
};

// One recognised line.  The optional fields are filled only when the request asks for them: nothing extra is launched or
// allocated otherwise.
struct RecResult {
    RecLine line;
    uint32_t ctc_len = 0;            // the model's sequence length for the line (ctc_input_len); 0: the line gave no input
    std::vector<CtcStep> steps;
    // Recognition confidence (DESIGN.md "Recognition confidence"), scored requests: each step's log-prob L[pos][label],
    // indexed like the steps, and the line score (greedy: the float64 sum of the masked row maxima in ascending t; beam:
    // the best beam's lse(pb, pnb)).  A line without rows has no steps and score 0.
    std::vector<float> step_logp;
    double line_score = 0.0;
    // when asked: the model's log-probabilities [ctc_len][C] (TextRecognizer::run, recognition.rs:341-360), unmasked
    std::vector<float> logp;
};

// Test hook (ocrs_ctc_decode_packed): the decode stage of a packed recognition batch on chosen head outputs.  `logits`: the
// n lines' rows [T[i]][C], line after line; `excluded`: [C] flags or null; method 0 greedy, 1 greedy scored, 2 beam search
// on the GPU, 3 the same scored.  The lines are planned by HipModel::make_packed_plan and laid out at rows off[t] + m as a
// request's are, then go through log_softmax_argmax and the engine's own decode_packed (engine.cpp).  res: one result per
// line in the caller's order — steps, step_logp / line_score (scored), logp (want_logp; unmasked), ctc_len; a line with T = 0 stays empty.
void ctc_decode_packed(const float* logits, const int32_t* T, size_t n, int C, const uint8_t* excluded, int method,
                       uint32_t width, bool want_logp, std::vector<RecResult>* res);

// Test hook (ocrs_mask_component_rects): the component stage of detection (detection.rs:41-62) on chosen masks [n][h][w]
// (0 / 1 bytes, host).  The masks are uploaded and run through k::ccl_label and k::contour_rects as run_ccl runs an unscored,
// unprepared size group (eps 2, the process's ccl_quad option, buffers from alloc_ccl) with the caller's expand, min_area,
// max_comp and arena.  Out, per page: n_roots, the overflow flag, rects [max_comp][6] and valid [max_comp]; a slot the
// contour kernel did not write holds valid 0xEE and all-ones rect words.
void mask_component_rects(const uint8_t* masks, int n, int h, int w, float expand, float min_area, int max_comp, int64_t arena,
                          int32_t* n_roots, int32_t* overflow, float* rects, uint8_t* valid);

// One line to crop into a tensor of recognition inputs: rows of `out_w` floats, the first at float offset `out_off`.
struct CropLine {
    const RecLine* line;
    uint32_t out_w;
    int64_t out_off;
};
// Builds the crop descriptors of `crops`, uploads them through `ws` and launches the crops (plain and rectified lines: one
// launch each) into a new tensor of `total` floats, which it returns; null when there is nothing to crop.
float* stage_line_crops(Workspace& ws, StageTimers* timers, const ocrs_page* const* pages, size_t n_pages,
                        const std::vector<CropLine>& crops, int rec_h, int64_t total);

// Detection confidence, indexed [page][word] like the rects of the same call.
struct DetScores {
    std::vector<std::vector<float>> score;      // mean text probability of the word's component, from the fixed-point sum
    std::vector<std::vector<uint32_t>> pixels;  // pixels of that component
};

// Tiled detection: the plan along one axis of page length L for a model of length M and overlap v,
// 0 <= v <= M / 2.  L <= M: one tile.  Else n = ceil((L - v) / (M - v)) tiles with origins (i * (L - M)) / (n - 1) — the first at 0,
// the last ending at L — and ownership bounds in the middle of the neighbours' overlaps: tile i owns [bound[i], bound[i + 1]).
struct TileAxisPlan {
    std::vector<int32_t> origin;   // [n]
    std::vector<int32_t> bound;    // [n + 1], bound[0] = 0, bound[n] = L
};
TileAxisPlan tile_axis_plan(int L, int M, int v);

// One caller's detection / recognition request while it waits in the engine's coalescer (coalesce.hpp).
struct DetRequest : CoalescedBase {
    const ocrs_page* const* pages = nullptr;
    size_t n = 0;
    std::vector<std::vector<geom::RotatedRect>>* rects = nullptr;
    DetScores* scores = nullptr;   // null: the caller did not ask for confidence
};
struct RecRequest : CoalescedBase {
    const ocrs_page* const* pages = nullptr;
    size_t n_pages = 0;
    const std::vector<std::vector<std::vector<geom::RotatedRect>>>* lines_per_page = nullptr;
    std::vector<RecResult>* results = nullptr;
    bool scored = false;           // the caller asked for confidence
    bool rectify = false;          // this caller's lines are cropped along their own axes
};

}  // namespace ocrs

struct ocrs_engine {
    int device = 0;   // the HIP device of its models (ocrs_engine_new); every call binds the calling thread to it
    const ocrs::ModelBase* detection = nullptr;
    const ocrs::ModelBase* recognition = nullptr;
    bool debug = false;
    ocrs_decode_method decode_method = OCRS_DECODE_GREEDY;
    uint32_t beam_width = 100;
    std::u32string alphabet;
    bool has_excluded = false;
    std::vector<uint8_t> excluded;  // [alphabet_len + 1] flags by label
    ocrs::DevBuf d_excluded;
    // TextDetectorParams::default() (detection.rs:25-37)
    float min_area = 100.0f;
    float text_threshold = 0.2f;
    mutable ocrs::StageTimers timers;
    // the engine's copy of the tuning options (common.hpp): the process defaults at creation + ocrs_engine_params +
    // ocrs_engine_set_option; installed for the calling thread by every entry point (abi_util.hpp guarded_engine)
    ocrs::Tuning tuning{};
    // numerics != exact: the device context this engine is counted in (DeviceContext::add_relaxed_engine) — remembered, because
    // `device` may be reassigned after creation (a group member without weights) and the count must come off where it went on
    ocrs::DeviceContext* counted_relaxed = nullptr;
    void count_relaxed(ocrs::DeviceContext& c) { uncount_relaxed(); c.add_relaxed_engine(+1); counted_relaxed = &c; }
    void uncount_relaxed() noexcept {
        if (!counted_relaxed) return;
        try { counted_relaxed->add_relaxed_engine(-1); } catch (...) {}
        counted_relaxed = nullptr;
    }
    ~ocrs_engine() { uncount_relaxed(); }

    ocrs::StageTimers* tm() const { return timers.enabled ? &timers : nullptr; }

    // detection.rs:104-200 over a batch of equally sized pages.  Small requests (fewer pages than half of option
    // "coalesce_pages") that only want rects are merged with concurrent ones (coalesce.hpp); results are those of
    // detect_now on the caller's pages alone.
    // scores (optional, with rects): per word the component's score and pixel count; null allocates and launches nothing extra.
    // tile_overlap >= 0: tiled detection with that overlap — pages are cut into model-sized tiles at their own
    // resolution instead of being resized; such a request is never merged with others.  < 0: the untiled call.
    void detect(const ocrs_page* const* pages, size_t n, std::vector<std::vector<ocrs::geom::RotatedRect>>* rects,
                float* host_map /* [n,h,w] or null */, ocrs::DetScores* scores = nullptr, int tile_overlap = -1) const;
    void detect_now(const ocrs_page* const* pages, size_t n, std::vector<std::vector<ocrs::geom::RotatedRect>>* rects,
                    float* host_map, ocrs::DetScores* scores = nullptr, int tile_overlap = -1) const;

    // recognition.rs:404-540 over the lines of several pages; small requests are merged likewise.
    // rectify: the request's lines are cropped along their own axes; a merged batch may mix both kinds.
    void recognize(const ocrs_page* const* pages, size_t n_pages,
                   const std::vector<std::vector<std::vector<ocrs::geom::RotatedRect>>>& lines_per_page,
                   std::vector<ocrs::RecResult>* results, bool scored = false, bool rectify = false) const;
    // want_logp: every line's model output too.  rectify_pages (optional): one flag per page, the kind of that page's
    // lines; null: all plain.  Lines beyond the activation budget run as consecutive sub-requests.
    void recognize_now(const ocrs_page* const* pages, size_t n_pages,
                       const std::vector<std::vector<std::vector<ocrs::geom::RotatedRect>>>& lines_per_page,
                       std::vector<ocrs::RecResult>* results, bool scored = false, bool want_logp = false,
                       const std::vector<char>* rectify_pages = nullptr) const;
    void init_coalescers();
    mutable std::unique_ptr<ocrs::Coalescer<ocrs::DetRequest>> det_queue;
    mutable std::unique_ptr<ocrs::Coalescer<ocrs::RecRequest>> rec_queue;
    // one sub-request of `recognize_now` (within the activation budget): fills the `n` fresh results at `res`, whose `line`s are set
    void recognize_lines(const ocrs_page* const* pages, size_t n_pages, ocrs::RecResult* res, size_t n, bool scored,
                         bool want_logp) const;
    // the recognition model's output for the lines of one page, no coalescing (parity / tolerance checks); split into
    // sub-requests within the activation budget as `recognize` is
    void recognize_logits(const ocrs_page* page, const std::vector<std::vector<ocrs::geom::RotatedRect>>& lines,
                          std::vector<std::vector<float>>* logp, int* classes) const;
    // test hook (ocrs_engine_run_recognition_ops): ops [first_op, last_op] of the recognition model through
    // run_recognition_packed, over lines of model-input widths `widths`.  `in`: op first_op's input, line after line in the
    // oracle's per-line layout ([H][W][C] in the conv stack and at the TOSEQ, [T][1][C] after it); `out` likewise for op
    // last_op's output ([2][T][3H]: gx_only, a GRU's input projections), `shapes` three dims per line.
    void run_recognition_ops(const int32_t* widths, size_t n, int first_op, int last_op, bool gx_only, const float* in,
                             size_t in_len, std::vector<float>* out, std::vector<int32_t>* shapes) const;

    // char_logp (optional, scored results): receives the log-prob of every char's step, aligned with the result
    std::vector<ocrs::TextChar> text_line_from_result(const ocrs::RecResult& res, std::vector<float>* char_logp = nullptr) const;

    uint32_t rec_input_height() const;
    ocrs::RecLine make_rec_line(const std::vector<ocrs::geom::RotatedRect>& words, size_t page, size_t index,
                                bool rectify = false) const;
};
