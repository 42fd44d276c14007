// The ragged recognition batch: all width groups of a request through the conv stack at once (run_prefix_ragged), then the
// packed rows through the GRU layers, the Linear and the LogSoftmax (run_recognition_packed).
#include <functional>
#include <mutex>

#include "model_exec.hpp"
#include "ragged_plan.hpp"

namespace ocrs {

namespace {
// supported stack: CONV 3x3 (Cin == 1 directly followed by MAXPOOL 2x2, or Cin % 32 == 0), MAXPOOL, AVGPOOL,
// each consuming the previous op's output
bool ragged_stack_supported(const std::vector<GraphOp>& ops, int ts, int h) {
    for (int i = 0; i < ts; i++) {
        const GraphOp& op = ops[i];
        if (op.in0 != (i == 0 ? 0 : ops[i - 1].out)) return false;
        if (op.type == OP_CONV) {
            if (op.kh != 3 || op.kw != 3 || !op.relu) return false;
            if (op.cin == 1) {
                if (i + 1 >= ts || ops[i + 1].type != OP_MAXPOOL || ops[i + 1].kh != 2 || ops[i + 1].kw != 2) return false;
                if (op.cout > 64 || op.cout < 4 || (op.cout & (op.cout - 1)) != 0) return false;  // 4, 8, 16, 32, 64
            } else if ((op.cin % 32) != 0 || op.cout < 64 || (op.cout % 4) != 0) {
                return false;
            }
        } else if (op.type != OP_MAXPOOL && op.type != OP_AVGPOOL) {
            return false;
        }
    }
    // the patch-tiled conv needs H % 4 == 0 at every Cin > 1 conv
    for (int i = 0; i < ts; i++) {
        if (ops[i].type == OP_CONV && ops[i].cin != 1 && (h % 4) != 0) return false;
        if (ops[i].type == OP_MAXPOOL || ops[i].type == OP_AVGPOOL) h /= ops[i].kh;
    }
    return true;
}

// The activation buffers of one conv-stack run.
// On the device's shared conv-stack stream the intermediate activations come from the DEVICE's arena instead of the
// request's workspace: they are touched only by kernels of that one stream, which run in the order they were enqueued
// (under heavy_phase, held since before_launch), so every request's stack can use the same few buffers — with
// six 16-page requests in flight that is ~5 GB once instead of ~5 GB per request.  Buffers are never handed back while
// the process runs (an earlier request's kernels may still be using them); the arena grows to the largest request seen.
struct StackBuffers {
    Workspace& ws;
    const bool shared_arena;
    std::vector<std::pair<float*, size_t>> spare;  // released buffers, reused by later layers
    std::vector<char> arena_taken;
    float* held = nullptr;   // the buffer holding the current activations (nullptr: the caller's input)
    size_t held_bytes = 0;

    float* get(size_t floats) {
        const size_t bytes = floats * sizeof(float);
        for (size_t i = 0; i < spare.size(); i++)
            if (spare[i].second >= bytes) { float* p = spare[i].first; spare.erase(spare.begin() + i); return p; }
        if (!shared_arena) return static_cast<float*>(ws.alloc(bytes));
        auto& arena = ctx().heavy_arena;
        arena_taken.resize(arena.size(), 0);
        size_t best = arena.size();
        for (size_t i = 0; i < arena.size(); i++)
            if (!arena_taken[i] && arena[i].bytes >= bytes && (best == arena.size() || arena[i].bytes < arena[best].bytes)) best = i;
        if (best == arena.size()) {
            arena.emplace_back(bytes + bytes / 8);   // a little head-room: requests of a stream differ by a few lines
            arena_taken.push_back(0);
        }
        arena_taken[best] = 1;
        return arena[best].as<float>();
    }
    // y (from get) holds the current activations now: what held them before is free for later layers
    void rotate(float* y, size_t floats) {
        if (held) spare.emplace_back(held, held_bytes);
        held = y; held_bytes = floats * sizeof(float);
    }
};

// The launches of the ragged conv stack, ops [0, ts), or of the op range [first, last] of it.
struct RaggedStack {
    const HipModel& m;
    const RaggedPlan& geo;
    StageTimers* timers;
    hipStream_t st;
    const int ts, first, last;
    StackBuffers bufs;
    const float* cur;   // the current activations
    int curC = 1;

    template <class Launch>
    void timed(int cls, double flops, double bytes, Launch&& launch) { timed_launch(timers, st, cls, flops, bytes, launch); }
    // an op range (test hook): the launches before it are planned, not run, and none may straddle either end of it
    bool launches(int i, int j) const {   // the launch of ops [i, j] runs?
        if (i < first && j >= first)
            fail(OCRS_ERR_INVALID_ARGUMENT, "op range: op %d lies inside the fused launch of ops %d..%d (a range starts at %d)", first, i, j, i);
        if (i <= last && j > last)
            fail(OCRS_ERR_INVALID_ARGUMENT, "op range: op %d lies inside the fused launch of ops %d..%d (a range ends at %d)", last, i, j, j);
        return i >= first;
    }
    float* output(const k::RaggedView& vout, int c) { return bufs.get((size_t)vout.pixels * c); }
    void produced(float* y, const k::RaggedView& vout, int c) {
        bufs.rotate(y, (size_t)vout.pixels * c);
        cur = y;
    }

    // The launch that starts at op i; returns the last op it covers (ts: the AvgPool that ends the stack, left to finish()).
    int step(int i) {
        const auto& ops = m.ops;
        const GraphOp& op = ops[i];
        const k::RaggedView vin = geo.view(i);
        if (op.type == OP_CONV && op.cin == 1) {
            // conv1 + pool + conv2 + pool in one kernel where the shapes allow (kernels_rec.hip: conv12_fused_ragged)
            if (i + 3 < ts && ops[i + 2].type == OP_CONV && ops[i + 2].cin == op.cout && ops[i + 2].relu &&
                ops[i + 3].type == OP_MAXPOOL && ops[i + 3].kh == 2 && ops[i + 3].kw == 2) {
                const GraphOp& op2 = ops[i + 2];
                const k::RaggedView vmid = geo.view(i + 2), vout = geo.view(i + 4);
                if (k::conv12_fused_ragged(nullptr, vin, vmid, nullptr, nullptr, op.cout, nullptr, nullptr, op2.cout, nullptr, vout, st)) {
                    if (launches(i, i + 3)) {
                        float* y = output(vout, op2.cout);
                        // counted as conv2's launch with conv2's FLOPs (the matrix-core work); conv1's VALU work rides along
                        timed(KC_GEMM_CONV3X3, 2.0 * vmid.pixels * 9.0 * op2.cin * op2.cout,
                              4.0 * (vin.pixels + vout.pixels * op2.cout) + 4.0 * op2.wcount[0],
                              [&] { k::conv12_fused_ragged(cur, vin, vmid, op.w[0], op.w[1], op.cout, op2.w[0], op2.w[1], op2.cout, y, vout, st, op2.wsplit); });
                        produced(y, vout, op2.cout);
                    }
                    curC = op2.cout;
                    return i + 3;
                }
            }
            const k::RaggedView vout = geo.view(i + 2);  // after the fused MaxPool 2x2
            if (launches(i, i + 1)) {
                float* y = output(vout, op.cout);
                timed(KC_CONV_DIRECT, 2.0 * vin.pixels * 9 * op.cout, 4.0 * vin.pixels + 4.0 * vout.pixels * op.cout,
                      [&] { k::conv1_relu_pool_ragged(cur, vin, op.w[0], op.w[1], op.cout, y, vout, st); });
                produced(y, vout, op.cout);
            }
            curC = op.cout;
            return i + 1;  // the pool is fused
        }
        if (op.type == OP_CONV) {
            // a MaxPool 2x1 / 2x2 that consumes this conv is folded into its epilogue
            const bool fuse = i + 1 < ts && ops[i + 1].type == OP_MAXPOOL && ops[i + 1].kh == 2 &&
                              (ops[i + 1].kw == 1 || ops[i + 1].kw == 2) && vin.H % 2 == 0;
            const int ph = fuse ? 2 : 1, pw = fuse ? ops[i + 1].kw : 1;
            const k::RaggedView vout = geo.view(fuse ? i + 2 : i + 1);
            if (launches(i, fuse ? i + 1 : i)) {
                float* y = output(vout, op.cout);
                bool ok = false;
                timed(KC_GEMM_CONV3X3, 2.0 * vin.pixels * 9.0 * op.cin * op.cout,
                      4.0 * (vin.pixels * op.cin + vout.pixels * op.cout) + 4.0 * op.wcount[0],
                      [&] { ok = k::conv3x3_ragged(cur, vin, op.cin, op.w[0], op.w[1], op.cout, op.relu, ph, pw, y, vout, st, op.wsplit, op.skip_exact); });
                if (!ok) fail(OCRS_ERR_RUN_FAILED, "model run failed: ragged conv %d->%d at height %d not supported", op.cin, op.cout, vin.H);
                produced(y, vout, op.cout);
            }
            curC = op.cout;
            return fuse ? i + 1 : i;
        }
        if (op.type == OP_AVGPOOL && i + 1 == ts && op.kw == 1 && op.kh == vin.H && (curC & 3) == 0) {
            launches(i, ts);
            return ts;   // the column average down to height 1 that ends the stack: done together with the sequence packing
        }
        if (launches(i, i)) {
            const k::RaggedView vout = geo.view(i + 1);
            float* y = output(vout, curC);
            timed(KC_POOL, 0, 4.0 * curC * (vin.pixels + vout.pixels),
                  [&] { k::pool_ragged(cur, vin, curC, op.kh, op.kw, op.type == OP_AVGPOOL, y, vout, st); });
            produced(y, vout, curC);
        }
        return i;
    }

    // What the run hands back, in the request's own workspace: the packed feature rows of the whole stack, or (the range
    // ended at op `at` inside the stack) that op's output out of the (possibly shared) arena.
    float* finish(int at, Workspace& ws, const HipModel::PackedPlan& plan, const int32_t* d_pos) {
        if (at < ts) {
            float* X = ws.alloc_n<float>(bufs.held_bytes / sizeof(float));
            OCRS_HIP(hipMemcpyAsync(X, bufs.held, bufs.held_bytes, hipMemcpyDeviceToDevice, st));
            return X;
        }
        const auto& ops = m.ops;
        const k::RaggedView vf = geo.view(ts);
        if (vf.H != 1) fail(OCRS_ERR_RUN_FAILED, "model run failed: TOSEQ expects height 1, got %d", vf.H);
        float* X = ws.alloc_n<float>((size_t)plan.R * curC);
        const bool pool_here = ts >= 1 && ops[ts - 1].type == OP_AVGPOOL && ops[ts - 1].kw == 1 && (curC & 3) == 0 &&
                               ops[ts - 1].kh == geo.view(ts - 1).H;
        if (pool_here) {
            const k::RaggedView vp = geo.view(ts - 1);
            timed(KC_POOL, 0, 4.0 * curC * (vp.pixels + vf.pixels),
                  [&] { k::avgpool_to_seq_ragged(cur, vp, vf, curC, d_pos, plan.d_off, X, st); });
        } else {
            launches(ts, ts);
            timed(KC_OTHER, 0, 8.0 * vf.pixels * curC, [&] { k::to_seq_packed_ragged(cur, vf, curC, d_pos, plan.d_off, X, st); });
        }
        return X;
    }
};
}  // namespace

float* HipModel::run_prefix_ragged(Workspace& ws, hipStream_t exec, const std::vector<PackedGroup>& groups,
                                   const PackedPlan& plan, int h, int ts, StageTimers* timers, int* feat_c,
                                   const std::function<void()>& before_launch, const OpRange* range,
                                   hipEvent_t* stack_done) const {
    const int G = (int)groups.size();
    if (G == 0 || ts <= 0 || !ragged_stack_supported(ops, ts, h)) return nullptr;
    // groups must be contiguous in memory (an op range that starts later hands in one ragged buffer: groups[0].d_batch)
    for (int g = 0; g + 1 < G && !(range && range->first > 0); g++)
        if (groups[g].d_batch + (size_t)groups[g].n * h * groups[g].w != groups[g + 1].d_batch) return nullptr;

    // ---- per-layer geometry on the host, one metadata upload
    RaggedPlan geo(ops, ts, h, groups);
    int64_t* d64 = ws.alloc_n<int64_t>(geo.meta64.size());
    int32_t* d32 = ws.alloc_n<int32_t>(geo.meta32.size());
    ws.upload(d64, geo.meta64.data(), geo.meta64.size() * sizeof(int64_t));
    ws.upload(d32, geo.meta32.data(), geo.meta32.size() * sizeof(int32_t));
    geo.d64 = d64;
    geo.d32 = d32;
    if (before_launch) before_launch();   // everything above is host work and uploads on the request's own stream
    if (exec != ws.s()) {  // inputs (crops, plan, metadata) were produced on the request's stream: light-lane work, runnable
                           // as queued, so the conv lane may wait for it on the device (the same wait on the host, ahead of
                           // heavy_phase, measured 0.3 % lower: profiles/stream_budget_cost.txt)
        hipEvent_t ready = ws.make_event();
        OCRS_HIP(hipEventRecord(ready, ws.s()));
        OCRS_HIP(hipStreamWaitEvent(exec, ready, 0));
    }

    int tok = timers ? timers->begin(ST_REC_CONV, exec, 0) : -1;
    // (a request of a device that runs one kernel at a time — StreamLease::serial() — has exec == its own stream: it shares
    // the arena all the same)
    const bool shared_arena = exec != ws.s() || (ws.stream.serial() && before_launch);
    RaggedStack stack{*this, geo, timers, exec, ts, range ? range->first : 0, range ? range->last : ts,
                      StackBuffers{ws, shared_arena}, groups[0].d_batch};
    int at = ts;   // the op at which the stack stopped (ts: all of it ran)
    for (int i = 0; i < ts; i++) {
        i = stack.step(i);
        if (i >= stack.last) { at = i; break; }
    }
    float* X = stack.finish(at, ws, plan, groups[0].d_pos);
    if (tok >= 0) timers->end(tok, exec);
    if (exec != ws.s()) {  // the request continues once the conv stack has drained
        hipEvent_t done = ws.make_event();
        OCRS_HIP(hipEventRecord(done, exec));
        // A lane shared with other calls never has a wait for the conv lane parked in it (stream_plan.hpp): the caller's
        // host thread waits for `done`, once it has let go of heavy_phase, and enqueues what follows when it wakes.
        if (stack_done && !ws.stream.may_park_waits()) *stack_done = done;
        else OCRS_HIP(hipStreamWaitEvent(ws.s(), done, 0));
    }
    *feat_c = stack.curC;
    return X;
}

const int32_t* HipModel::make_packed_plan(Workspace& ws, const std::vector<int32_t>& T, PackedPlan* plan,
                                          std::vector<size_t>* order) {
    order->clear();
    for (size_t i = 0; i < T.size(); i++)
        if (T[i] > 0) order->push_back(i);
    std::stable_sort(order->begin(), order->end(), [&](size_t a, size_t b) { return T[a] > T[b]; });
    const int M = (int)order->size();
    if (M == 0) return nullptr;
    plan->M = M;
    plan->Tmax = T[(*order)[0]];
    plan->active.assign(plan->Tmax, 0);
    std::vector<int32_t> hTm(M), hoff(plan->Tmax + 1, 0), hpos(T.size(), 0);
    for (int m = 0; m < M; m++) {
        hTm[m] = T[(*order)[m]];
        hpos[(*order)[m]] = m;
        for (int t = 0; t < hTm[m]; t++) plan->active[t]++;
    }
    for (int t = 0; t < plan->Tmax; t++) hoff[t + 1] = hoff[t] + plan->active[t];
    plan->R = hoff[plan->Tmax];
    std::vector<int32_t> meta(hTm);   // Tm | off | pos
    meta.insert(meta.end(), hoff.begin(), hoff.end());
    meta.insert(meta.end(), hpos.begin(), hpos.end());
    int32_t* d_meta = ws.alloc_n<int32_t>(meta.size());
    ws.upload(d_meta, meta.data(), meta.size() * sizeof(int32_t));
    plan->d_Tm = d_meta;
    plan->d_off = d_meta + M;
    plan->h_Tm = std::move(hTm);
    plan->h_off = std::move(hoff);
    return d_meta + M + plan->Tmax + 1;
}

int HipModel::packed_split() const {
    int ts = -1;
    for (size_t i = 0; i < ops.size(); i++)
        if (ops[i].type == OP_TOSEQ) { ts = (int)i; break; }
    if (ts < 0 || (size_t)ts + 3 > ops.size()) return -1;
    int prev_out = ops[ts].out;
    for (size_t i = ts + 1; i < ops.size(); i++) {
        const GraphOp& op = ops[i];
        const bool last = i + 1 == ops.size(), second_last = i + 2 == ops.size();
        if (op.in0 != prev_out) return -1;
        if (last) { if (op.type != OP_LOGSOFTMAX || (uint32_t)op.out != out_slot) return -1; }
        else if (second_last) { if (op.type != OP_LINEAR) return -1; }
        else if (op.type != OP_GRU) return -1;
        prev_out = op.out;
    }
    for (int i = 0; i < ts; i++)
        if (ops[i].type == OP_GRU || ops[i].type == OP_LINEAR || ops[i].type == OP_LOGSOFTMAX || ops[i].type == OP_TOSEQ)
            return -1;
    return ts;
}

namespace {
// One run_recognition_packed call: the packed rows `cur` [R][curC] on their way through the ops after the conv stack.
struct PackedRun {
    const HipModel& m;
    Workspace& ws;
    const HipModel::PackedPlan& plan;
    StageTimers* timers;
    HipModel::OpRange* range;
    hipStream_t st;
    const float* cur = nullptr;
    int curC = 0;
    int gru_layer = 0;
    float* gx_buf = nullptr; size_t gx_cap = 0;   // one buffer of input projections for all layers
    void* hx_buf = nullptr;   // the recurrences' hand-off buffer: likewise one for all layers (a layer's marks are written after the
    size_t hx_cap = 0;        // previous layer's recurrence has finished: this stream waits for it)

    template <class Launch>
    void timed(int cls, double flops, double bytes, Launch&& launch) { timed_launch(timers, st, cls, flops, bytes, launch); }
    int begin(int stage) { return timers ? timers->begin(stage, st, 0) : -1; }
    void end(int tok) { if (tok >= 0) timers->end(tok, st); }

    // Conv stack -> packed feature rows, one launch per layer over all groups (ragged); nullptr if the stack has an op the
    // ragged kernels do not cover.
    // The conv stack saturates the GPU; the recurrence that follows is a chain of small,
    // latency-bound launches.  When several requests are in flight (host threads / streams),
    // two conv stacks at once gain nothing, but a conv stack next to other requests' GRU chains
    // does: so every request's conv stack is enqueued on one shared stream (FIFO on the GPU, linked
    // to the request's own stream by events) and everything after it overlaps freely.
    float* run_conv_stack(const std::vector<HipModel::PackedGroup>& groups, int h, int ts, int* C0) {
        // all conv stacks of a device go through ONE stream, in request order.  The lock is taken by the hook, i.e. after
        // the request's geometry has been worked out and its metadata uploads are queued.
        std::unique_lock<std::mutex> heavy(ctx().heavy_phase, std::defer_lock);
        const hipStream_t conv = ws.stream.conv_stream();   // the device's conv-stack stream
        hipEvent_t stack_done = nullptr;
        float* X = nullptr;
        try {
            X = m.run_prefix_ragged(ws, conv, groups, plan, h, ts, timers, C0, [&] { heavy.lock(); }, range, &stack_done);
        } catch (...) {
            // Kernels of this request may already be queued on the shared stream, reading and writing scratch
            // that ~Workspace hands back to the pool after waiting only for what the request queued on its OWN
            // stream: wait for them first (best effort, no throw on the error path) — on the host, with heavy_phase
            // released, so that nothing is parked in a lane that other calls share.
            hipEvent_t e = nullptr;
            const bool recorded = hipEventCreateWithFlags(&e, hipEventBlockingSync | hipEventDisableTiming) == hipSuccess &&
                                  hipEventRecord(e, conv) == hipSuccess;
            if (e) ws.events.push_back(e);
            if (heavy.owns_lock()) heavy.unlock();
            if (!recorded || wait_event(e) != hipSuccess) (void)hipStreamSynchronize(conv);
            throw;
        }
        if (heavy.owns_lock()) heavy.unlock();
        if (stack_done) ws.host_wait(stack_done);
        return X;
    }

    // ... or group by group through run_device, each group's features packed into the rows; nullptr without groups
    float* run_groups_unpacked(const std::vector<HipModel::PackedGroup>& groups, int h, int ts, int* C0) {
        float* X = nullptr;
        for (const HipModel::PackedGroup& g : groups) {
            TensorShape fs;
            float* feat = m.run_device(ws, g.d_batch, g.n, h, g.w, &fs, timers, nullptr, nullptr, true, false, ts);
            if (fs.h != 1) fail(OCRS_ERR_RUN_FAILED, "model run failed: TOSEQ expects height 1, got %d", fs.h);
            if (!X) {
                *C0 = fs.c;
                X = ws.alloc_n<float>((size_t)plan.R * fs.c);
            }
            int tok = begin(ST_REC_CONV);
            timed(KC_OTHER, 0, 8.0 * fs.count(), [&] { k::to_seq_packed(feat, g.n, fs.w, fs.c, g.d_pos, plan.d_off, X, st); });
            end(tok);
        }
        return X;
    }

    // ONE launch for all Tmax steps of both directions (kernels_gru.hip).  Its workgroups wait on
    // each other, so two such kernels must never be half-resident at the same time: every request's
    // recurrences go through one stream per device (FIFO on the GPU, linked by events, no host wait).
    // np: 0, or the bf16 planes of the state (kernels_gru_split.hip).  false: the kernel has no plan for this shape.
    bool gru_persistent_launch(const GraphOp& op, const float* gx, float* y, void* hx, int np) {
        const int H = op.hidden, M = plan.M;
        const int64_t R = plan.R;
        uint32_t* d_sync = ws.alloc_n<uint32_t>(k::gru_persistent_sync_words(M));
        double fl = 0.0;
        for (int step = 0; step < plan.Tmax; step++) fl += 2.0 * 2 * plan.active[step] * 3.0 * H * H;
        bool ran = false;
        hipEvent_t rec_done = nullptr;
        {
            std::lock_guard<std::mutex> g(ctx().rec_phase);
            hipStream_t rs = ws.stream.recurrent_stream();
            hipEvent_t ready = ws.make_event(), done = ws.make_event();
            OCRS_HIP(hipEventRecord(ready, st));
            OCRS_HIP(hipStreamWaitEvent(rs, ready, 0));
            timed_launch(timers, rs, KC_GEMM_GRU_HIDDEN, fl, 4.0 * ((double)R * (2.0 * 3 * H + 2.0 * 2 * H) + 2.0 * 3 * H * H), [&] {
                ran = np ? k::gru_persistent_split(gx, op.aux2, op.aux3, y, static_cast<uint16_t*>(hx), plan.d_Tm, plan.d_off, plan.h_Tm.data(), R, M, plan.Tmax, H, np, d_sync, rs)
                         : k::gru_persistent(gx, op.aux2, op.aux3, y, static_cast<float*>(hx), plan.d_Tm, plan.d_off, plan.h_Tm.data(), R, M, plan.Tmax, H, d_sync, rs);
            });
            if (ran && plan.h_status && gru_layer < 8)
                ws.download(plan.h_status + gru_layer, d_sync + k::gru_persistent_sync_words(M) - 1, sizeof(uint32_t), rs);
            OCRS_HIP(hipEventRecord(done, rs));
            // the rest of the request follows the recurrence: a wait parked in the request's own stream, or on a
            // lane shared with other calls a wait of the host thread (below, rec_phase released)
            if (rs == st || ws.stream.may_park_waits()) OCRS_HIP(hipStreamWaitEvent(st, done, 0));
            else rec_done = done;
        }
        if (rec_done) ws.host_wait(rec_done);
        return ran;
    }

    // One launch per time step (option gru_mode = 1, and shapes the persistent kernel has no plan for):
    // hidden GEMM + gates in one kernel, transposed ping-ponged state hT[2 dirs][H][Mcap].
    void gru_steps_fused(const GraphOp& op, const float* gx, float* y) {
        const int H = op.hidden, Mcap = (plan.M + 3) & ~3;
        float* hT0 = ws.alloc_n<float>((size_t)2 * H * Mcap);
        float* hT1 = ws.alloc_n<float>((size_t)2 * H * Mcap);
        OCRS_HIP(hipMemsetAsync(hT0, 0, (size_t)2 * H * Mcap * sizeof(float), st));
        for (int step = 0; step < plan.Tmax; step++) {
            const int act = plan.active[step];
            if (act <= 0) break;
            const float* hin = (step & 1) ? hT1 : hT0;
            float* hout = (step & 1) ? hT0 : hT1;
            timed(KC_GEMM_GRU_HIDDEN, 2.0 * 2 * act * 3.0 * H * H,
                  4.0 * 2 * ((double)act * H * 2 + (double)act * 3 * H + 3.0 * H * H + (double)act * H), [&] {
                      if (!k::gru_step_fused(gx, op.aux2, op.aux3, hin, hout, y, plan.d_Tm, plan.d_off, plan.R, Mcap, act, H, step, st))
                          fail(OCRS_ERR_RUN_FAILED, "model run failed: no fused GRU step kernel for hidden size %d", H);
                  });
        }
    }

    // any other hidden size: hidden GEMM and gate kernel as two launches per time step
    void gru_steps_unfused(const GraphOp& op, const float* gx, float* y) {
        const int H = op.hidden, M = plan.M;
        float* gh = ws.alloc_n<float>((size_t)2 * M * 3 * H);
        float* hs = ws.alloc_n<float>((size_t)2 * M * H);
        OCRS_HIP(hipMemsetAsync(hs, 0, (size_t)2 * M * H * sizeof(float), st));
        k::GemmDesc r = desc::gru_hidden(op, hs, gh, M);
        for (int step = 0; step < plan.Tmax; step++) {
            const int act = plan.active[step];
            if (act <= 0) break;
            r.M = act;
            timed(KC_GEMM_GRU_HIDDEN, 2.0 * 2 * act * (double)r.N * r.K,
                  4.0 * 2 * ((double)act * r.K + (double)act * r.N + (double)r.K * r.N), [&] { k::gemm(r, st); });
            timed(KC_GRU_GATES, 0, 4.0 * 2 * act * (double)H * 9,
                  [&] { k::gru_gates_packed(gx, gh, hs, y, plan.d_Tm, plan.d_off, plan.R, M, act, H, step, st); });
        }
    }

    // Input projections of all rows, then the recurrence.  false: the range asked for the projections only (range->out).
    bool run_gru_layer(const GraphOp& op, bool is_last) {
        const int H = op.hidden, I = op.cin, M = plan.M;
        const int64_t R = plan.R;
        if (I != curC) fail(OCRS_ERR_RUN_FAILED, "model run failed: GRU input size %d != %d", I, curC);
        int tok = begin(ST_REC_GRU);
        // the input projections of a layer are dead once its recurrence has run, and the next layer's projection is
        // ordered after that recurrence (it reads its output): one buffer serves every layer (2.3 GB per layer at 16 pages)
        const size_t gx_floats = (size_t)2 * R * 3 * H;
        if (gx_floats > gx_cap) { gx_buf = ws.alloc_n<float>(gx_floats); gx_cap = gx_floats; }
        float* gx = gx_buf;
        float* y = ws.alloc_n<float>((size_t)R * 2 * H);
        const bool fused = (H == 256 || H == 128 || H == 64);
        const bool persistent = fused && gru_mode() == GRU_PERSISTENT && k::gru_persistent_supported(plan.h_Tm.data(), M, plan.Tmax, R, H);
        // numerics != exact: the recurrence on the bf16 matrix cores (kernels_gru_split.hip), state cut into 3 / 2 planes
        int np = option(OPT_NUMERICS) == 1 ? 3 : option(OPT_NUMERICS) == 2 ? 2 : 0;
        if (!(persistent && np != 0 && k::gru_split_supported(plan.h_Tm.data(), M, plan.Tmax, R, H, np))) np = 0;
        // the hand-off buffer of the launch, every word marked "unwritten" ahead of the input GEMM
        const size_t hx_bytes = np ? k::gru_split_exchange_bytes(plan.h_Tm.data(), M, H, np) : persistent ? k::gru_persistent_exchange_bytes(plan.h_Tm.data(), M, H) : 0;
        if (hx_bytes > hx_cap) { hx_buf = ws.alloc(hx_bytes); hx_cap = hx_bytes; }
        if (np) OCRS_HIP(k::gru_split_prepare(static_cast<uint16_t*>(hx_buf), plan.h_Tm.data(), M, H, np, st));
        else if (persistent) OCRS_HIP(k::gru_persistent_prepare(static_cast<float*>(hx_buf), plan.h_Tm.data(), M, H, st));
        const k::GemmDesc d = desc::gru_input(op, cur, gx, R, true);
        // (round 3's option gx_heavy queued these projections on the conv-stack stream: every MFMA class then ran at its
        // alone speed at the same or slightly lower pages/s — a zero-sum trade, removed in round 5)
        timed(KC_GEMM_GRU_INPUT, 2.0 * 2 * R * (double)d.N * d.K, 4.0 * ((double)R * I + 2.0 * R * d.N + 2.0 * d.K * d.N),
              [&] { k::gemm(d, st); });
        if (range && range->gx_only && is_last) {
            range->out = gx; range->out_c = 3 * H;
            return false;
        }
        if (!(persistent && gru_persistent_launch(op, gx, y, hx_buf, np))) {
            if (fused) gru_steps_fused(op, gx, y);
            else gru_steps_unfused(op, gx, y);
        }
        end(tok);
        gru_layer++;
        cur = y;
        curC = 2 * H;
        return true;
    }

    void run_linear(const GraphOp& op) {
        const int64_t R = plan.R;
        if (op.cin != curC) fail(OCRS_ERR_RUN_FAILED, "model run failed: Linear input size %d != %d", op.cin, curC);
        int tok = begin(ST_REC_HEAD);
        float* y = ws.alloc_n<float>((size_t)R * op.cout);
        const k::GemmDesc d = desc::dense(op, cur, y, R);
        timed(KC_GEMM_LINEAR, 2.0 * R * (double)d.N * d.K, 4.0 * ((double)R * (op.cin + op.cout)) + 4.0 * op.wcount[0],
              [&] { k::gemm(d, st); });
        end(tok);
        cur = y;
        curC = op.cout;
    }

    // LOGSOFTMAX (+ arg-max); returns the class count
    int run_log_softmax(const uint8_t* d_excluded, int32_t* d_labels, float** d_logp, float* d_maxlp) {
        const int64_t R = plan.R;
        int tok = begin(ST_REC_HEAD);
        float* lp = nullptr;
        if (d_logp || range) {
            lp = ws.alloc_n<float>((size_t)R * curC);
            if (d_logp) *d_logp = lp;
        }
        timed(KC_LOGSOFTMAX_ARGMAX, 0, 4.0 * R * curC * (lp ? 2.0 : 1.0), [&] {
            if (!k::log_softmax_argmax(cur, R, curC, d_excluded, lp, d_labels, st, d_maxlp))
                fail(OCRS_ERR_CAPACITY, "LogSoftmax over %d classes exceeds the kernel's LDS staging (max ~630)", curC);
        });
        end(tok);
        if (range) cur = lp;
        return curC;
    }
};
}  // namespace

int HipModel::run_recognition_packed(Workspace& ws, const std::vector<PackedGroup>& groups, const PackedPlan& plan, int h,
                                     StageTimers* timers, const uint8_t* d_excluded, int32_t* d_labels,
                                     float** d_logp, float* d_maxlp, OpRange* range) const {
    const int ts = packed_split();
    if (ts < 0) fail(OCRS_ERR_RUN_FAILED, "model run failed: graph is not <conv stack> TOSEQ GRU* LINEAR LOGSOFTMAX");
    const int first = range ? range->first : 0, last = range ? range->last : (int)ops.size() - 1;
    PackedRun run{*this, ws, plan, timers, range, ws.s()};
    if (first <= ts) {
        int C0 = 0;
        float* X = run.run_conv_stack(groups, h, ts, &C0);
        if (range) {
            if (!X) fail(OCRS_ERR_INVALID_ARGUMENT, "op range: this model's conv stack has no ragged form");
            if (last < ts) {
                range->out = X; range->out_c = C0;
                return 0;
            }
        }
        if (!X) X = run.run_groups_unpacked(groups, h, ts, &C0);
        if (!X) return 0;
        run.cur = X; run.curC = C0;
    } else {
        run.cur = range->seq_in; run.curC = range->in_c;
    }
    int classes = 0;
    for (int i = std::max(ts + 1, first); i <= last; i++) {
        const GraphOp& op = ops[i];
        if (op.type == OP_LINEAR) run.run_linear(op);
        else if (op.type == OP_LOGSOFTMAX) classes = run.run_log_softmax(d_excluded, d_labels, d_logp, d_maxlp);
        else if (!run.run_gru_layer(op, i == last)) return 0;
    }
    if (range) { range->out = run.cur; range->out_c = run.curC; }
    OCRS_HIP(hipGetLastError());
    return classes;
}

}  // namespace ocrs
