// HipModel::run_device: one forward of the op graph on one stream, op by op, the activations recycled by liveness.
// (model_load.cpp builds the graph; model_packed.cpp is the ragged recognition batch.)
#include <cstdio>
#include <map>

#include "model_exec.hpp"

namespace ocrs {

namespace {
// The activation buffer of every slot during one forward; the buffers of dead slots serve later ones.
struct SlotTable {
    using Buf = std::pair<float*, size_t>;   // pointer, capacity in bytes
    Workspace& ws;
    std::vector<float*> ptr;
    std::vector<size_t> cap;      // 0: not this table's to release (the caller's input)
    std::vector<int> last_use;    // last op index that reads each slot
    std::multimap<size_t, float*> free_list;

    SlotTable(Workspace& w, size_t n_slots) : ws(w), ptr(n_slots, nullptr), cap(n_slots, 0), last_use(n_slots, -1) {}
    Buf get(size_t floats) {   // a scratch buffer: put() it back after use
        size_t bytes = floats * sizeof(float);
        auto it = free_list.lower_bound(bytes);
        if (it != free_list.end() && it->first <= bytes * 2 + 4096) {
            Buf r{it->second, it->first};
            free_list.erase(it);
            return r;
        }
        size_t rounded = (bytes + 255) & ~size_t(255);
        return {static_cast<float*>(ws.alloc(rounded)), rounded};
    }
    void put(Buf b) { free_list.emplace(b.second, b.first); }
    float* bind(int slot, size_t floats) {
        Buf r = get(floats);
        ptr[slot] = r.first; cap[slot] = r.second;
        return r.first;
    }
    void alias(int out, int in) {   // `out` takes over the buffer of `in`
        ptr[out] = ptr[in]; cap[out] = cap[in];
        ptr[in] = nullptr; cap[in] = 0;
    }
    void release_if_last(int sl, int i) {
        if (sl > 0 && last_use[sl] == i && ptr[sl] && cap[sl]) {   // slot 0 is the caller's
            put({ptr[sl], cap[sl]});
            ptr[sl] = nullptr; cap[sl] = 0;
        }
    }
    // release those of `slots` whose last reader op i was
    void release_after(size_t i, std::initializer_list<int> slots) {
        for (int sl : slots) release_if_last(sl, (int)i);
    }
    // ... and any slot at all (after a fused launch: incl. a skipped PADCAT's inputs)
    void release_all_after(size_t i) {
        for (int sl = 1; sl < (int)ptr.size(); sl++) release_if_last(sl, (int)i);
    }
};

// Model.run(timing=True): one event behind every op, and the table printed from them.
struct OpEvents {
    std::vector<hipEvent_t> ev;
    OpEvents(bool on, size_t n_ops, hipStream_t st) {
        if (!on) return;
        ev.resize(n_ops + 1);
        for (auto& e : ev) OCRS_HIP(hipEventCreate(&e));
        OCRS_HIP(hipEventRecord(ev[0], st));
    }
    ~OpEvents() { for (auto& e : ev) (void)hipEventDestroy(e); }
    void mark(size_t i, hipStream_t st) { if (!ev.empty()) OCRS_HIP(hipEventRecord(ev[i + 1], st)); }
    void print(const HipModel& m, const std::vector<TensorShape>& shp, size_t n_run, hipStream_t st) {
        if (ev.empty()) return;
        OCRS_HIP(hipStreamSynchronize(st));
        float total = 0.f;
        for (size_t i = 0; i < n_run; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            total += ms;
            const TensorShape o = shp[m.ops[i].out];
            printf("%-10s [%d,%d,%d,%d] %.3fms\n", kOpNames[m.ops[i].type], o.n, o.h, o.w, o.c, ms);
        }
        printf("total %.3fms\n", total);
    }
};

// The state of one run_device call and the launch of every op family.
struct DeviceRun {
    const HipModel& m;
    StageTimers* timers;
    hipStream_t st;
    std::vector<TensorShape> shp;
    TensorShape out;
    size_t n_run;        // ops [0, n_run) run
    uint32_t ret_slot;   // the slot this run returns
    SlotTable slots;
    std::vector<char> covered;   // ops already done by a fused DoubleConv launch
    int stage_token = -1, cur_stage = -1;
    bool seen_seq = false;

    DeviceRun(const HipModel& model, Workspace& ws, int n, int h, int w, StageTimers* t, int stop_before, hipStream_t s)
        : m(model), timers(t), st(s), slots(ws, model.n_slots), covered(model.ops.size(), 0) {
        const auto& ops = m.ops;
        out = m.infer(n, h, w, &shp);
        n_run = stop_before >= 0 ? (size_t)stop_before : ops.size();
        ret_slot = stop_before >= 0 ? (uint32_t)ops[stop_before].in0 : m.out_slot;
        if (stop_before >= 0) out = shp[ret_slot];
        std::vector<int>& last_use = slots.last_use;
        for (size_t i = 0; i < ops.size(); i++) {
            last_use[ops[i].in0] = (int)i;
            if (ops[i].in1 >= 0) last_use[ops[i].in1] = (int)i;
        }
        last_use[m.out_slot] = (int)ops.size() + 1;
        last_use[ret_slot] = (int)ops.size() + 1;
        for (size_t i = 0; i + 1 < ops.size(); i++)
            if (cat_fused(i)) {   // the op after the skipped PADCAT reads its inputs
                last_use[ops[i].in0] = std::max(last_use[ops[i].in0], (int)i + 1);
                last_use[ops[i].in1] = std::max(last_use[ops[i].in1], (int)i + 1);
            }
    }
    // PADCAT i is skipped and op i+1 reads its inputs (only inside this run's range)
    bool cat_fused(size_t i) const { return m.ops[i].cat_into_next && i + 1 < n_run && (int)ret_slot != m.ops[i].out; }
    template <class Launch>
    void timed(int cls, double flops, double bytes, Launch&& launch, double mfma_flops = -1.0) {
        timed_launch(timers, st, cls, flops, bytes, launch, mfma_flops);
    }

    // one stage per op, chosen once: detection graphs are one stage; recognition graphs switch at TOSEQ
    void enter_stage_of(const GraphOp& op) {
        int stage = ST_DET_CNN;
        if (m.kind != 0) {
            if (op.type == OP_GRU) stage = ST_REC_GRU;
            else if (op.type == OP_LINEAR || op.type == OP_LOGSOFTMAX) stage = seen_seq ? ST_REC_HEAD : ST_REC_CONV;
            else stage = seen_seq ? ST_REC_GRU : ST_REC_CONV;
        }
        if (op.type == OP_TOSEQ) seen_seq = true;
        if (!timers || stage == cur_stage) return;
        leave_stage();
        stage_token = timers->begin(stage, st, 0);
        cur_stage = stage;
    }
    void leave_stage() { if (timers && cur_stage >= 0) timers->end(stage_token, st); }

    // The fused launch of DoubleConv block b, if this run may fuse it and a kernel takes this request; marks the ops it covers.
    bool double_conv_block(const DcBlock& b) {
        const auto& ops = m.ops;
        if ((size_t)b.last >= n_run) return false;
        for (int q = b.first; q < b.last; q++)   // no intermediate may be what this run returns
            if ((uint32_t)ops[q].out == ret_slot && q != b.pw2) return false;
        if (b.fin >= 0 && (uint32_t)ops[b.pw2].out == ret_slot) return false;
        const GraphOp &d1 = ops[b.dw1], &p1 = ops[b.pw1], &d2 = ops[b.dw2], &p2 = ops[b.pw2];
        const int skip_slot = b.cat >= 0 ? ops[b.cat].in0 : d1.in0;
        const TensorShape sk = shp[skip_slot];
        k::DoubleConvArgs da{};
        da.skip = slots.ptr[skip_slot];
        da.n = sk.n; da.h = sk.h; da.w = sk.w;
        double px1 = 0;
        if (b.convt >= 0) {
            const GraphOp& ct = ops[b.convt];
            const TensorShape x1 = shp[ct.in0];
            da.x1 = slots.ptr[ct.in0]; da.h1 = x1.h; da.w1 = x1.w;
            da.wt = ct.w[0]; da.bt = ct.w[1];
            px1 = (double)x1.n * x1.h * x1.w;
            if (2 * x1.h > sk.h || 2 * x1.w > sk.w) return false;
        }
        da.wd1 = d1.w[0]; da.bd1 = d1.w[1]; da.wp1 = p1.w[0]; da.bp1 = p1.w[1];
        da.wd2 = d2.w[0]; da.bd2 = d2.w[1]; da.wp2 = p2.w[0]; da.bp2 = p2.w[1];
        da.relu_d1 = d1.relu; da.relu_p1 = p1.relu; da.relu_d2 = d2.relu; da.relu_p2 = p2.relu;
        da.tape = b.tape; da.tape_len = b.tape_len; da.rtape = b.rtape; da.rtape_len = b.rtape_len;
        // Is there a fused kernel for THIS request (its page count and sizes, not just the block's channel counts)?  A
        // query with the real arguments: the row-streaming kernels decline some requests (more than 8 pages, an odd pad
        // offset) and the next kernel family takes them; a block that no fused kernel takes falls through to the
        // per-operator kernels.
        bool on_mfma = false;
        int path = 0;   // which kernel family will take it (nothing is launched by the query)
        if (!k::double_conv_fused(da, b.cs, b.cx, b.cmid, b.cout, b.pool >= 0, b.fin >= 0, false, nullptr, &on_mfma, &path)) return false;
        double out_floats = 0;
        auto output = [&](int slot) {
            out_floats += (double)shp[slot].count();
            return slots.bind(slot, (size_t)shp[slot].count());
        };
        if (b.fin >= 0) {
            da.y = output(b.sig >= 0 ? ops[b.sig].out : ops[b.fin].out);
            da.wf = ops[b.fin].w[0]; da.bf = ops[b.fin].w[1]; da.sigmoid = b.sig >= 0;
        } else {
            da.y = output(p2.out);
            if (b.pool >= 0) da.ypool = output(ops[b.pool].out);
        }
        const int cin = d1.cin;
        const double px = (double)sk.n * sk.h * sk.w;
        const double fl = 2.0 * px * (9.0 * cin + (double)cin * b.cmid + 9.0 * b.cmid + (double)b.cmid * b.cout +
                                      (b.fin >= 0 ? b.cout : 0)) + 2.0 * px * (b.convt >= 0 ? (double)b.cx * b.cs : 0.0);
        // of which dense contractions (pointwise convs, ConvTranspose) — on the matrix cores if the block's MFMA variant runs
        const double fl_dense = 2.0 * px * ((double)cin * b.cmid + (double)b.cmid * b.cout) +
                                2.0 * px * (b.convt >= 0 ? (double)b.cx * b.cs : 0.0);
        bool launched = false;
        timed(path == 1 ? KC_DET_STREAM_WAVE : path == 2 ? KC_DET_STREAM_ROWS : KC_DET_BLOCK, fl, 4.0 * (px * b.cs + px1 * b.cx + out_floats), [&] {
            launched = k::double_conv_fused(da, b.cs, b.cx, b.cmid, b.cout, b.pool >= 0, b.fin >= 0, true, st);
        }, on_mfma ? fl_dense : 0.0);
        if (!launched) fail(OCRS_ERR_RUN_FAILED, "model run failed: internal (no fused kernel took the DoubleConv block its query accepted)");
        for (int q = b.first + 1; q <= b.last; q++) covered[q] = 1;
        return true;
    }

    void conv(size_t i, const TensorShape& a, const float* x, float* y) {
        const GraphOp& op = m.ops[i];
        const int64_t px = (int64_t)a.n * a.h * a.w;
        const bool next_sigmoid = i + 1 < m.ops.size() && m.ops[i + 1].fused_into_prev;
        const double cflops = 2.0 * px * op.cout * op.cin * op.kh * op.kw;
        const double cbytes = 4.0 * (double)px * (op.cin + op.cout) + weight_bytes(op, 0);
        if (op.kh == 1 && op.kw == 1 && op.cout == 1) {
            timed(KC_CONV1X1_SIGMOID, cflops, cbytes,
                  [&] { k::conv1x1_cout1(x, px, op.cin, op.w[0], op.w[1], op.relu, next_sigmoid ? 1 : 0, y, st); });
        } else if (op.kh == 1 && op.kw == 1 && (op.cin % 4) == 0) {
            timed(KC_GEMM_POINTWISE, cflops, cbytes, [&] { k::gemm(desc::dense(op, x, y, px), st); });
        } else if (op.kh == 3 && op.kw == 3 && (op.cin % 32) == 0) {
            timed(KC_GEMM_CONV3X3, cflops, cbytes, [&] { k::gemm(desc::conv3x3(op, x, y, a), st); });
        } else if ((op.cout % 4) == 0) {
            timed(KC_CONV_DIRECT, cflops, cbytes, [&] {
                k::conv_direct(x, a.n, a.h, a.w, op.cin, op.w[0], op.w[1], op.kh, op.kw, op.cout, op.relu, y, st);
            });
        } else {
            fail(OCRS_ERR_RUN_FAILED, "model run failed: unsupported conv shape %dx%d %d->%d", op.kh, op.kw,
                 op.cin, op.cout);
        }
    }

    // depthwise 3x3 + pointwise 1x1 as one kernel: writes the pointwise conv's output
    void dwconv_pw(const GraphOp& op, const GraphOp& pw, const TensorShape& a, const float* x) {
        float* y = slots.bind(pw.out, (size_t)shp[pw.out].count());
        const double px = (double)a.n * a.h * a.w;
        timed(KC_DWCONV3X3, 2.0 * px * (9.0 * op.cin + (double)op.cin * pw.cout), 4.0 * px * (op.cin + pw.cout), [&] {
            k::dwpw_fused(x, a.n, a.h, a.w, op.cin, op.w[0], op.w[1], op.relu, pw.cout, pw.w[0], pw.w[1], pw.relu, y, st);
        });
    }
    void dwconv(const GraphOp& op, const TensorShape& a, const float* x, float* y) {
        timed(KC_DWCONV3X3, 18.0 * a.count(), 8.0 * a.count(),
              [&] { k::dwconv3x3(x, a.n, a.h, a.w, a.c, op.w[0], op.w[1], op.relu, y, st); });
    }
    // depthwise 3x3 over the two inputs of the skipped PADCAT i - 1
    void dwconv_cat(size_t i, const TensorShape& a, float* y) {
        const GraphOp &op = m.ops[i], &cat = m.ops[i - 1];
        const TensorShape sk = shp[cat.in0], up = shp[cat.in1];
        const float *skip = slots.ptr[cat.in0], *upx = slots.ptr[cat.in1];
        if ((sk.c % 4) == 0 && (up.c % 4) == 0) {
            timed(KC_DWCONV3X3, 18.0 * a.count(), 8.0 * a.count(), [&] {
                k::dwconv3x3_cat(skip, sk.n, sk.h, sk.w, sk.c, upx, up.h, up.w, up.c, op.w[0], op.w[1], op.relu, y, st);
            });
        } else {  // channel counts the vectorised kernel does not take: build the concatenation after all
            auto tmp = slots.get((size_t)a.count());
            timed(KC_PADCAT, 0, 8.0 * a.count(),
                  [&] { k::padcat(skip, sk.n, sk.h, sk.w, sk.c, upx, up.h, up.w, up.c, tmp.first, st); });
            dwconv(op, a, tmp.first, y);
            slots.put(tmp);
        }
        slots.release_after(i, {cat.in0, cat.in1});   // the skipped PADCAT's inputs: this was their last reader
    }

    // the GRU of the unpacked path: input projections of all steps, then hidden GEMM + gates per time step
    void gru(const GraphOp& op, const TensorShape& a, const float* x, float* y) {
        const int T = a.n, N = a.h, H = op.hidden;
        auto gx = slots.get((size_t)2 * T * N * 3 * H);
        auto gh = slots.get((size_t)2 * N * 3 * H);
        auto hs = slots.get((size_t)2 * N * H);
        OCRS_HIP(hipMemsetAsync(hs.first, 0, (size_t)2 * N * H * sizeof(float), st));
        const k::GemmDesc d = desc::gru_input(op, x, gx.first, (int64_t)T * N, false);
        timed(KC_GEMM_GRU_INPUT, 2.0 * 2 * d.M * (double)d.N * d.K,
              4.0 * ((double)a.count() + 2.0 * d.M * d.N + 2.0 * d.K * d.N), [&] { k::gemm(d, st); });
        const k::GemmDesc r = desc::gru_hidden(op, hs.first, gh.first, N);
        for (int step = 0; step < T; step++) {
            timed(KC_GEMM_GRU_HIDDEN, 2.0 * 2 * r.M * (double)r.N * r.K,
                  4.0 * 2 * ((double)r.M * r.K + (double)r.M * r.N + (double)r.K * r.N), [&] { k::gemm(r, st); });
            timed(KC_GRU_GATES, 0, 4.0 * 2 * N * (double)H * 9,
                  [&] { k::gru_gates(gx.first, gh.first, hs.first, y, T, N, H, step, st); });
        }
        slots.put(gx); slots.put(gh); slots.put(hs);
    }

    void run_op(size_t i, const uint8_t* d_excluded, int32_t* d_labels, bool want_logp) {
        const GraphOp& op = m.ops[i];
        const TensorShape a = shp[op.in0], o = shp[op.out];
        const float* x = slots.ptr[op.in0];
        if (op.fused_into_prev) return slots.alias(op.out, op.in0);   // already holds sigmoid(conv)
        if (op.type == OP_PADCAT && cat_fused(i)) return;   // the depthwise conv that follows reads skip / up directly
        if (op.done_by_prev && slots.ptr[op.out]) return;   // computed together with the preceding depthwise conv
        if (op.fuse_next_pw && !op.reads_cat && i + 1 < n_run && (int)ret_slot != op.out) return dwconv_pw(op, m.ops[i + 1], a, x);
        const bool is_final_logsoftmax = op.type == OP_LOGSOFTMAX && (uint32_t)op.out == m.out_slot;
        float* y = is_final_logsoftmax && !want_logp ? nullptr : slots.bind(op.out, (size_t)o.count());
        switch (op.type) {
            case OP_CONV: conv(i, a, x, y); break;
            case OP_DWCONV3:
                if (op.reads_cat && i > 0 && cat_fused(i - 1)) dwconv_cat(i, a, y);
                else dwconv(op, a, x, y);
                break;
            case OP_MAXPOOL: case OP_AVGPOOL:
                timed(KC_POOL, 0, 4.0 * (a.count() + o.count()),
                      [&] { (op.type == OP_MAXPOOL ? k::maxpool : k::avgpool)(x, a.n, a.h, a.w, a.c, op.kh, op.kw, y, st); });
                break;
            case OP_CONVT2: {
                const k::GemmDesc d = desc::convt(op, x, y, a);
                timed(KC_GEMM_CONVT, 2.0 * d.M * op.cin * op.cout * 4, 4.0 * (a.count() + o.count()) + weight_bytes(op, 0),
                      [&] { k::gemm(d, st); });
                break;
            }
            case OP_PADCAT: {
                const TensorShape b = shp[op.in1];
                timed(KC_PADCAT, 0, 8.0 * o.count(),
                      [&] { k::padcat(x, a.n, a.h, a.w, a.c, slots.ptr[op.in1], b.h, b.w, b.c, y, st); });
                break;
            }
            case OP_SIGMOID: timed(KC_OTHER, 0, 8.0 * a.count(), [&] { k::sigmoid(x, y, a.count(), st); }); break;
            case OP_TOSEQ:
                if (a.h != 1) fail(OCRS_ERR_RUN_FAILED, "model run failed: TOSEQ expects height 1, got %d", a.h);
                timed(KC_OTHER, 0, 8.0 * a.count(), [&] { k::to_seq(x, a.n, a.w, a.c, y, st); });
                break;
            case OP_GRU: gru(op, a, x, y); break;
            case OP_LINEAR: {
                const k::GemmDesc d = desc::dense(op, x, y, (int64_t)a.n * a.h * a.w);
                timed(KC_GEMM_LINEAR, 2.0 * d.M * (double)d.N * d.K, 4.0 * ((double)a.count() + o.count()) + weight_bytes(op, 0),
                      [&] { k::gemm(d, st); });
                break;
            }
            case OP_LOGSOFTMAX:
                timed(KC_LOGSOFTMAX_ARGMAX, 0, 4.0 * a.count() * (y ? 2.0 : 1.0), [&] {
                    if (!k::log_softmax_argmax(x, (int64_t)a.n * a.h * a.w, a.c, is_final_logsoftmax ? d_excluded : nullptr, y,
                                               is_final_logsoftmax ? d_labels : nullptr, st))
                        fail(OCRS_ERR_CAPACITY, "LogSoftmax over %d classes exceeds the kernel's LDS staging (max ~630)", a.c);
                });
                break;
            default: fail(OCRS_ERR_RUN_FAILED, "model run failed: bad op");
        }
    }
};
}  // namespace

float* HipModel::run_device(Workspace& ws, const float* d_in, int n, int h, int w, TensorShape* out_shape,
                            StageTimers* timers, const uint8_t* d_excluded, int32_t* d_labels, bool want_logp,
                            bool print_timing, int stop_before, hipStream_t exec) const {
    hipStream_t st = exec ? exec : ws.s();
    DeviceRun run(*this, ws, n, h, w, timers, stop_before, st);
    if (out_shape) *out_shape = run.out;
    run.slots.ptr[0] = const_cast<float*>(d_in);
    OpEvents events(print_timing, ops.size(), st);
    const int det_fuse = option(OPT_DET_FUSE);
    for (size_t i = 0; i < run.n_run; i++) {
        const GraphOp& op = ops[i];
        run.enter_stage_of(op);
        if (run.covered[i] || (det_fuse && op.dc_block >= 0 && run.double_conv_block(dc_blocks[op.dc_block]))) {
            run.slots.release_all_after(i);
            events.mark(i, st);
            continue;
        }
        run.run_op(i, d_excluded, d_labels, want_logp);
        events.mark(i, st);
        run.slots.release_after(i, {op.in0, op.in1});   // inputs whose last reader this was
    }
    run.leave_stage();
    OCRS_HIP(hipGetLastError());
    events.print(*this, run.shp, run.n_run, st);
    return run.slots.ptr[run.ret_slot];
}

}  // namespace ocrs
