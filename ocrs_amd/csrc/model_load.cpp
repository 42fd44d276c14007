// Model files: HipModel::load (validate on the host, build and upload the weight slab, mark what run_device fuses),
// shape inference, and the caller-implemented model.
#include "conv_rows.hpp"
#include "model_exec.hpp"

namespace ocrs {

namespace {
#pragma pack(push, 1)
struct FileHeader {
    char magic[8];
    uint32_t version, kind;
    int64_t input_shape[4];
    uint32_t n_ops, n_slots, out_slot, reserved;
    uint64_t blob_floats;
};
struct FileOp {
    uint32_t type;
    int32_t in0, in1, out, relu, kh, kw, cin, cout, hidden;
    uint32_t n_w, reserved;
    struct { uint64_t off, cnt; } w[8];
};
#pragma pack(pop)
static_assert(sizeof(FileHeader) == 72, "header layout");
static_assert(sizeof(FileOp) == 176, "op layout");

struct ParsedFile {
    FileHeader hd;
    std::vector<FileOp> fops;
    const float* blob = nullptr;   // the file's weights (hd.blob_floats), in the caller's memory
    std::vector<float> slab;       // host image of the device slab: the file blob followed by derived tensors
};
struct Fix { size_t op; int which; size_t off; };   // derived tensor `which` (aux0..aux3) of an op, at slab offset `off`

void pad16(std::vector<float>& slab) { while (slab.size() % 4) slab.push_back(0.f); }

// A malformed or stale file must fail here, not index out of bounds in infer()/run_device() or on the device:
// slot numbers within the table, weight tensors of exactly the sizes the op's shape implies.
void check_op_record(const FileHeader& hd, const FileOp& f, uint32_t i) {
    if (f.type >= OP_COUNT || f.n_w > 8) fail(OCRS_ERR_IO, "bad op record %u", i);
    for (uint32_t j = 0; j < f.n_w; j++)
        if (f.w[j].off > hd.blob_floats || f.w[j].cnt > hd.blob_floats - f.w[j].off)
            fail(OCRS_ERR_IO, "weight reference out of range in op %u", i);
    const int64_t ns = hd.n_slots;
    const bool two_in = f.type == OP_PADCAT;
    if (f.in0 < 0 || f.in0 >= ns || f.out <= 0 || f.out >= ns || (two_in ? (f.in1 < 0 || f.in1 >= ns) : false) ||
        (!two_in && f.in1 >= ns))
        fail(OCRS_ERR_IO, "slot index out of range in op %u", i);
    auto want = [&](uint32_t j, int64_t cnt) {
        if (j >= f.n_w || cnt < 0 || (int64_t)f.w[j].cnt != cnt)
            fail(OCRS_ERR_IO, "op %u (%s): weight tensor %u has %llu floats, the op's shape needs %lld", i,
                 kOpNames[f.type], j, j < f.n_w ? (unsigned long long)f.w[j].cnt : 0ull, (long long)cnt);
    };
    auto pos = [&](int64_t v, const char* what) {
        if (v <= 0 || v > (1 << 20)) fail(OCRS_ERR_IO, "op %u (%s): bad %s %lld", i, kOpNames[f.type], what, (long long)v);
    };
    switch (f.type) {
        case OP_CONV: pos(f.kh, "kh"); pos(f.kw, "kw"); pos(f.cin, "cin"); pos(f.cout, "cout");
            want(0, (int64_t)f.kh * f.kw * f.cin * f.cout); want(1, f.cout); break;
        case OP_DWCONV3: pos(f.cin, "channels"); want(0, 9LL * f.cin); want(1, f.cin); break;
        case OP_MAXPOOL: case OP_AVGPOOL: pos(f.kh, "kh"); pos(f.kw, "kw"); break;
        case OP_CONVT2: pos(f.cin, "cin"); pos(f.cout, "cout"); want(0, 4LL * f.cin * f.cout); want(1, f.cout); break;
        case OP_GRU: pos(f.cin, "input size"); pos(f.hidden, "hidden size");
            if (f.n_w != 8) fail(OCRS_ERR_IO, "GRU op %u needs 8 weight tensors", i);
            for (uint32_t d = 0; d < 2; d++) {
                want(4 * d + 0, 3LL * f.cin * f.hidden); want(4 * d + 1, 3LL * f.hidden);
                want(4 * d + 2, 3LL * f.hidden * f.hidden); want(4 * d + 3, 3LL * f.hidden);
            }
            break;
        case OP_LINEAR: pos(f.cin, "cin"); pos(f.cout, "cout"); want(0, (int64_t)f.cin * f.cout); want(1, f.cout); break;
        default: break;
    }
}

// Channel counts, inferred statically: every input slot is the model input (slot 0, one channel) or the output of
// an earlier op, and every op with a `cin` reads a slot of exactly that many channels.  The kernels index their
// input with lda = cin; a mismatch or an unwritten slot would read out of bounds (or through a null pointer).
void check_channels(const FileHeader& hd, const std::vector<FileOp>& fops) {
    std::vector<int64_t> chans(hd.n_slots, -1);   // -1: not written yet
    chans[0] = 1;
    for (uint32_t i = 0; i < hd.n_ops; i++) {
        const FileOp& f = fops[i];
        auto in = [&](int32_t sl) {
            if (chans[sl] < 0)
                fail(OCRS_ERR_IO, "op %u (%s): input slot %d is not written by an earlier op", i, kOpNames[f.type], sl);
            return chans[sl];
        };
        const int64_t c0 = in(f.in0);
        auto need = [&](int64_t want, const char* what) {
            if (c0 != want)
                fail(OCRS_ERR_IO, "op %u (%s): %s is %lld but input slot %d carries %lld channels", i, kOpNames[f.type], what,
                     (long long)want, f.in0, (long long)c0);
        };
        int64_t co = c0;
        switch (f.type) {
            case OP_CONV: case OP_CONVT2: case OP_LINEAR: need(f.cin, "cin"); co = f.cout; break;
            case OP_DWCONV3: need(f.cin, "channels"); break;
            case OP_GRU: need(f.cin, "input size"); co = 2LL * f.hidden; break;
            case OP_PADCAT: co = c0 + in(f.in1); break;
            default: break;
        }
        if (co > (1 << 24)) fail(OCRS_ERR_IO, "op %u (%s): %lld output channels", i, kOpNames[f.type], (long long)co);
        chans[f.out] = co;
    }
    if (chans[hd.out_slot] < 0) fail(OCRS_ERR_IO, "the output slot %u is not written by any op", hd.out_slot);
}

// Host only (a malformed file fails before any device work): the checked op table and the slab holding the file's blob.
ParsedFile parse_and_validate(const void* data, size_t len) {
    ParsedFile pf;
    FileHeader& hd = pf.hd;
    if (len < sizeof(FileHeader)) fail(OCRS_ERR_IO, "model file too short");
    memcpy(&hd, data, sizeof hd);
    if (memcmp(hd.magic, "OCRSMDL1", 8) != 0 || hd.version != 1) fail(OCRS_ERR_IO, "not an OCRSMDL1 model file");
    if (hd.n_ops > (1u << 20) || hd.n_slots == 0 || hd.n_slots > (1u << 20) || hd.out_slot >= hd.n_slots)
        fail(OCRS_ERR_IO, "model file header out of range (%u ops, %u slots, output slot %u)", hd.n_ops, hd.n_slots, hd.out_slot);
    const size_t table = sizeof(FileHeader) + (size_t)hd.n_ops * sizeof(FileOp);
    if (len < table || hd.blob_floats > (len - table) / sizeof(float)) fail(OCRS_ERR_IO, "model file truncated");
    pf.blob = reinterpret_cast<const float*>(static_cast<const char*>(data) + table);
    pf.fops.resize(hd.n_ops);
    for (uint32_t i = 0; i < hd.n_ops; i++) {
        memcpy(&pf.fops[i], static_cast<const char*>(data) + sizeof(FileHeader) + (size_t)i * sizeof(FileOp), sizeof(FileOp));
        check_op_record(hd, pf.fops[i], i);
    }
    check_channels(hd, pf.fops);
    pf.slab.assign(pf.blob, pf.blob + hd.blob_floats);
    pad16(pf.slab);
    return pf;
}

GraphOp graph_op(const FileOp& f) {
    GraphOp op{};
    op.type = f.type; op.in0 = f.in0; op.in1 = f.in1; op.out = f.out;
    op.relu = f.relu; op.kh = f.kh; op.kw = f.kw; op.cin = f.cin; op.cout = f.cout; op.hidden = f.hidden;
    for (uint32_t j = 0; j < f.n_w; j++) op.wcount[j] = f.w[j].cnt;
    return op;
}

// Derived tensors, appended to the slab op by op: the ConvT weights as a GEMM operand, the GRU's two directions side by side.
std::vector<Fix> append_derived(ParsedFile& pf) {
    std::vector<Fix> fixes;
    std::vector<float>& slab = pf.slab;
    for (size_t i = 0; i < pf.fops.size(); i++) {
        const FileOp& f = pf.fops[i];
        if (f.type == OP_CONVT2) {
            // file: [2][2][Cin][Cout] -> GEMM B [Cin][(dy,dx,co)], bias repeated per (dy,dx)
            const float* w = pf.blob + f.w[0].off;
            const float* b = pf.blob + f.w[1].off;
            fixes.push_back({i, 0, slab.size()});
            for (int ci = 0; ci < f.cin; ci++)
                for (int q = 0; q < 4; q++)
                    for (int co = 0; co < f.cout; co++) slab.push_back(w[((size_t)q * f.cin + ci) * f.cout + co]);
            pad16(slab);
            fixes.push_back({i, 1, slab.size()});
            for (int q = 0; q < 4; q++)
                for (int co = 0; co < f.cout; co++) slab.push_back(b[co]);
            pad16(slab);
        } else if (f.type == OP_GRU) {
            // pack both directions contiguously: Wi [2][I][3H], bi [2][3H], Wh [2][H][3H], bh [2][3H]
            for (int part = 0; part < 4; part++) {
                fixes.push_back({i, part, slab.size()});
                for (int d = 0; d < 2; d++) {
                    const float* src = pf.blob + f.w[4 * d + part].off;
                    slab.insert(slab.end(), src, src + f.w[4 * d + part].cnt);
                }
                pad16(slab);
            }
        }
    }
    return fixes;
}

template <class T>
const T* upload_tape(HipModel& m, const std::vector<T>& host) {
    m.tapes.emplace_back(host.size() * sizeof(T));
    OCRS_HIP(hipMemcpy(m.tapes.back().p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return m.tapes.back().as<T>();
}

// The slab onto the device, and every op's weight and derived-tensor pointers into it.
void upload_slab(HipModel& m, const ParsedFile& pf, const std::vector<Fix>& fixes) {
    m.weights = DevBuf(pf.slab.size() * sizeof(float));
    OCRS_HIP(hipMemcpy(m.weights.p, pf.slab.data(), pf.slab.size() * sizeof(float), hipMemcpyHostToDevice));
    const float* base = m.weights.as<float>();
    for (size_t i = 0; i < m.ops.size(); i++)
        for (uint32_t j = 0; j < pf.fops[i].n_w; j++) m.ops[i].w[j] = base + pf.fops[i].w[j].off;
    for (const Fix& fx : fixes) {
        GraphOp& op = m.ops[fx.op];
        const float** aux[4] = {&op.aux0, &op.aux1, &op.aux2, &op.aux3};
        *aux[fx.which] = base + fx.off;
    }
}

// Relaxed numerics (ocrs_engine_params.numerics): the 3x3 convs of a recognition stack whose contraction can run on the
// bf16 matrix cores carry their weights a second time, cut into three bf16 terms in the kernel's LDS layout
// (split_mfma.hpp split_weights; 1.5x the fp32 bytes, a few MB per model).
void upload_split_images(HipModel& m, const ParsedFile& pf, const std::vector<Fix>& fixes) {
    const float* slab = pf.slab.data();
    for (size_t i = 0; i < m.ops.size(); i++) {
        GraphOp& op = m.ops[i];
        if (m.kind != 1 || op.type != OP_CONV || op.kh != 3 || op.kw != 3) continue;
        std::vector<uint16_t> img;
        if ((op.cin % 32) == 0 && (op.cout % 128) == 0)
            k::split_weights(slab + pf.fops[i].w[0].off, 9 * op.cin, op.cout, op.cout, &img);
        else if (op.cin == 32 && op.cout == 64)   // conv2 of the fused conv1 + conv2 launch: its own image (one tap per barrier)
            k::conv12_split_weights(slab + pf.fops[i].w[0].off, &img);
        else
            continue;
        op.wsplit = upload_tape(m, img);
    }
    // the same for the GRU input projections ([I][3H] per direction; derived tensor aux0 = [2][I][3H] in the slab)
    for (const Fix& fx : fixes) {
        GraphOp& op = m.ops[fx.op];
        if (fx.which != 0 || op.type != OP_GRU || (op.cin % 64) != 0 || ((3 * op.hidden) % 128) != 0) continue;
        std::vector<uint16_t> both;
        for (int dir = 0; dir < 2; dir++) {
            std::vector<uint16_t> img;
            k::split_weights(slab + fx.off + (size_t)dir * op.cin * 3 * op.hidden, op.cin, 3 * op.hidden, 3 * op.hidden, &img);
            both.insert(both.end(), img.begin(), img.end());
        }
        op.wsplit = upload_tape(m, both);
    }
}

// Option "conv_rows": which 3x3 convs may drop the matrix-core work of tap rows outside the image without changing a bit.
void mark_skip_exact(HipModel& m, const ParsedFile& pf) {
    for (size_t i = 0; i < m.ops.size(); i++) {
        GraphOp& op = m.ops[i];
        if (op.type != OP_CONV || op.kh != 3 || op.kw != 3) continue;
        const FileOp& f = pf.fops[i];
        op.skip_exact = conv_rows_skip_exact(pf.blob + f.w[0].off, f.w[0].cnt, pf.blob + f.w[1].off, f.w[1].cnt, op.relu != 0);
    }
}

// Pairs of neighbouring ops that run_device executes as one launch.
void mark_fusions(HipModel& m) {
    std::vector<GraphOp>& ops = m.ops;
    auto only_reader_is_next = [&](size_t i) {   // op i's output is read by op i + 1 and by nothing else
        const int slot = ops[i].out;
        if ((uint32_t)slot == m.out_slot) return false;
        for (size_t j = i + 2; j < ops.size(); j++)
            if (ops[j].in0 == slot || ops[j].in1 == slot) return false;
        return true;
    };
    for (size_t i = 0; i + 1 < ops.size(); i++) {
        GraphOp& a = ops[i];
        GraphOp& b = ops[i + 1];
        if (b.in0 != a.out) continue;
        const bool pw11 = b.type == OP_CONV && b.kh == 1 && b.kw == 1;
        // Fold SIGMOID into a directly preceding Cout==1 pointwise conv.
        if (a.type == OP_CONV && a.cout == 1 && a.kh == 1 && a.kw == 1 && b.type == OP_SIGMOID && only_reader_is_next(i))
            b.fused_into_prev = true;
        // Depthwise 3x3 followed by its pointwise 1x1 (both 8 <= C <= 32) run as one kernel.
        if (a.type == OP_DWCONV3 && pw11 && b.cin == a.cin && k::dwpw_fused_supported(a.cin, b.cout) && only_reader_is_next(i)) {
            a.fuse_next_pw = true; b.done_by_prev = true;
        }
        // PADCAT consumed only by the depthwise conv that follows: that conv reads skip / up directly.
        if (a.type == OP_PADCAT && b.type == OP_DWCONV3 && only_reader_is_next(i)) {
            a.cat_into_next = true; b.reads_cat = true;
        }
    }
}

// The row-streaming kernels for the block's shape: its weights laid out as the tapes a row step reads (kernels_det_stream.hip,
// kernels_det_rows.hip).
void upload_block_tapes(HipModel& m, const ParsedFile& pf, DcBlock& b) {
    auto host = [&](int op, int j) -> const float* { return op >= 0 ? pf.slab.data() + pf.fops[op].w[j].off : nullptr; };
    k::StreamWeights hw{host(b.convt, 0), host(b.convt, 1), host(b.dw1, 0), host(b.dw1, 1), host(b.pw1, 0), host(b.pw1, 1),
                        host(b.dw2, 0), host(b.dw2, 1), host(b.pw2, 0), host(b.pw2, 1), host(b.fin, 0), host(b.fin, 1)};
    k::DoubleConvArgs none{};
    std::vector<float> tape;
    int tape_len = 0;
    if (k::double_conv_stream(none, b.cs, b.cx, b.cmid, b.cout, b.pool >= 0, b.fin >= 0, false, nullptr, &hw, &tape, &tape_len)) {
        b.tape = upload_tape(m, tape);
        b.tape_len = tape_len;
    }
    if (k::double_conv_rows(none, b.cs, b.cx, b.cmid, b.cout, b.pool >= 0, b.fin >= 0, false, nullptr, &hw, &tape, &tape_len)) {
        b.rtape = upload_tape(m, tape);
        b.rtape_len = tape_len;
    }
}

// Whole DoubleConv blocks of the detection U-Net as one fused launch each (kernels_det.hip).
void find_double_conv_blocks(HipModel& m, const ParsedFile& pf) {
    auto& ops = m.ops;
    const int n = (int)ops.size();
    auto uses = [&](int slot) {
        int u = 0;
        for (const GraphOp& o : ops) u += (o.in0 == slot) + (o.in1 == slot);
        return u + ((uint32_t)slot == m.out_slot ? 1 : 0);
    };
    auto pw11 = [](const GraphOp& o) { return o.type == OP_CONV && o.kh == 1 && o.kw == 1; };
    for (int i = 0; i + 3 < n; i++) {
        DcBlock b;
        int j = i;
        if (ops[j].type == OP_CONVT2 && j + 1 < n && ops[j + 1].type == OP_PADCAT && ops[j + 1].in1 == ops[j].out &&
            uses(ops[j].out) == 1 && uses(ops[j + 1].out) == 1) {
            b.convt = j; b.cat = j + 1;
            j += 2;
        }
        if (j + 3 >= n) continue;
        const GraphOp &d1 = ops[j], &p1 = ops[j + 1], &d2 = ops[j + 2], &p2 = ops[j + 3];
        if (d1.type != OP_DWCONV3 || !pw11(p1) || d2.type != OP_DWCONV3 || !pw11(p2)) continue;
        if (b.cat >= 0 && d1.in0 != ops[b.cat].out) continue;
        if (p1.in0 != d1.out || d2.in0 != p1.out || p2.in0 != d2.out) continue;
        if (uses(d1.out) != 1 || uses(p1.out) != 1 || uses(d2.out) != 1) continue;
        if (p1.cin != d1.cin || d2.cin != p1.cout || p2.cin != d2.cin) continue;
        b.dw1 = j; b.pw1 = j + 1; b.dw2 = j + 2; b.pw2 = j + 3;
        b.first = i; b.last = j + 3;
        b.cmid = p1.cout; b.cout = p2.cout;
        if (b.convt >= 0) {
            b.cx = ops[b.convt].cin;
            b.cs = d1.cin - ops[b.convt].cout;
            if (b.cs != ops[b.convt].cout) continue;   // the kernels assume ConvT cout == skip channels
        } else {
            b.cs = d1.cin;
        }
        const int k = j + 4;
        if (k < n && ops[k].type == OP_MAXPOOL && ops[k].kh == 2 && ops[k].kw == 2 && ops[k].in0 == p2.out && b.convt < 0) {
            b.pool = k; b.last = k;
        } else if (k < n && pw11(ops[k]) && ops[k].cout == 1 && !ops[k].relu && ops[k].in0 == p2.out && uses(p2.out) == 1 && b.convt >= 0) {
            b.fin = k; b.last = k;
            if (k + 1 < n && ops[k + 1].type == OP_SIGMOID && ops[k + 1].fused_into_prev) { b.sig = k + 1; b.last = k + 1; }
            else if (uses(ops[k].out) == 0) continue;
        }
        k::DoubleConvArgs none{};   // is there a fused kernel for a block of this shape?  (nothing is launched by the query)
        if (!k::double_conv_fused(none, b.cs, b.cx, b.cmid, b.cout, b.pool >= 0, b.fin >= 0, false, nullptr)) continue;
        upload_block_tapes(m, pf, b);
        ops[i].dc_block = (int)m.dc_blocks.size();
        m.dc_blocks.push_back(b);
        i = b.last;   // blocks do not overlap
    }
}
}  // namespace

void CallbackModel::run(const float* input, const int64_t in_shape[4], std::vector<float>& out,
                        int64_t out_shape[4], int* out_ndim) const {
    float* o = nullptr;
    int64_t os[4] = {0, 0, 0, 0};
    int nd = 0;
    int rc = fn(user, input, in_shape, &o, os, &nd);
    if (rc != 0 || !o || nd < 1 || nd > 4) {
        if (o) free(o);
        fail(OCRS_ERR_RUN_FAILED, "model run failed: callback returned %d", rc);
    }
    int64_t cnt = 1;
    for (int i = 0; i < nd; i++) cnt *= os[i];
    out.assign(o, o + cnt);
    free(o);
    for (int i = 0; i < 4; i++) out_shape[i] = i < nd ? os[i] : 1;
    *out_ndim = nd;
}

std::unique_ptr<HipModel> HipModel::load(const void* data, size_t len, int device) {
    ParsedFile pf = parse_and_validate(data, len);
    const std::vector<Fix> fixes = append_derived(pf);
    auto m = std::make_unique<HipModel>();
    m->kind = pf.hd.kind;
    for (int i = 0; i < 4; i++) m->input_shape[i] = pf.hd.input_shape[i];
    m->n_slots = pf.hd.n_slots;
    m->out_slot = pf.hd.out_slot;
    for (const FileOp& f : pf.fops) m->ops.push_back(graph_op(f));
    // everything above is work on the host; from here on the thread is bound to the device that will hold the weights
    DeviceScope bind(device);
    m->device = ctx().device;
    upload_slab(*m, pf, fixes);
    upload_split_images(*m, pf, fixes);
    mark_skip_exact(*m, pf);
    mark_fusions(*m);
    find_double_conv_blocks(*m, pf);
    return m;
}

TensorShape HipModel::infer(int n, int h, int w, std::vector<TensorShape>* slots_out) const {
    std::vector<TensorShape> s(n_slots);
    s[0] = TensorShape{n, h, w, 1, false};
    for (const GraphOp& op : ops) {
        const TensorShape a = s[op.in0];
        TensorShape o = a;
        switch (op.type) {
            case OP_CONV: o.c = op.cout; break;
            case OP_MAXPOOL:
            case OP_AVGPOOL: o.h = a.h / op.kh; o.w = a.w / op.kw; break;
            case OP_CONVT2: o.h = 2 * a.h; o.w = 2 * a.w; o.c = op.cout; break;
            case OP_PADCAT: o.c = a.c + s[op.in1].c; break;
            case OP_DWCONV3: case OP_SIGMOID: case OP_LOGSOFTMAX: break;
            case OP_TOSEQ: o = TensorShape{a.w, a.n, 1, a.c, true}; break;  // [T,N,C]
            case OP_GRU: o.c = 2 * op.hidden; break;
            case OP_LINEAR: o.c = op.cout; break;
            default: fail(OCRS_ERR_IO, "bad op type %u", op.type);
        }
        s[op.out] = o;
    }
    TensorShape out = s[out_slot];
    if (slots_out) *slots_out = std::move(s);
    return out;
}

double HipModel::flops(int n, int h, int w) const {
    std::vector<TensorShape> s;
    infer(n, h, w, &s);
    double total = 0;
    for (const GraphOp& op : ops) {
        const TensorShape a = s[op.in0];
        const double px = (double)a.n * a.h * a.w;
        switch (op.type) {
            case OP_CONV: total += 2.0 * px * op.cout * op.cin * op.kh * op.kw; break;
            case OP_DWCONV3: total += 2.0 * px * a.c * 9; break;
            case OP_CONVT2: total += 2.0 * px * op.cin * op.cout * 4; break;
            case OP_GRU: total += 2.0 * 2.0 * px * 3 * op.hidden * (op.cin + op.hidden); break;
            case OP_LINEAR: total += 2.0 * px * op.cin * op.cout; break;
            default: break;
        }
    }
    return total;
}

}  // namespace ocrs
