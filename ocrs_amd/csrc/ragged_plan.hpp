// Geometry of the ragged recognition conv stack (model_packed.cpp): every layer's image sizes and the cumulative tile
// tables its kernels search, built on the host into two blobs that are uploaded once.  No HIP call in here.
#pragma once
#include <algorithm>

#include "kernels.hpp"
#include "model.hpp"

namespace ocrs {

struct RaggedPlan {
    struct Table { size_t off = 0; int32_t total = 0; };   // a cumulative table [G+1] in meta32, and its last entry
    struct Layer {
        int H = 0;
        std::vector<int32_t> W;
        size_t w = 0, p = 0;      // W [G] in meta32, pixel offsets [G+1] in meta64
        Table t256;               // 256-pixel tiles
        Table t32, t16;           // 4 x 32 and 8 x 16 pixel patches (conv3x3_ragged)
        Table f32[2], f16[2];     // the same patches over the group's whole strip of images; [1]: image widths rounded up to even
        Table gap;                // 8 x 16 patches, images one empty column (at least) apart (conv12_fused_ragged)
        int64_t pixels = 0;
    };
    int G = 0;
    std::vector<int32_t> n;       // images per group
    std::vector<Layer> layers;    // [0]: the input; [i + 1]: the output of op i
    // n [G] | loff [G+1] | per layer: W [G] | t256 | t32 | t16 | gap | f32[0] | f16[0] | f32[1] | f16[1]
    std::vector<int32_t> meta32;
    std::vector<int64_t> meta64;  // per layer: poff [G+1]
    size_t loff_at = 0;
    const int32_t* d32 = nullptr;   // where the kernels read the two blobs: set by whoever uploads them
    const int64_t* d64 = nullptr;

    RaggedPlan(const std::vector<GraphOp>& ops, int ts, int h, const std::vector<HipModel::PackedGroup>& groups)
        : G((int)groups.size()) {
        Layer in;
        in.H = h;
        for (const HipModel::PackedGroup& g : groups) { n.push_back(g.n); in.W.push_back(g.w); }
        layers.push_back(std::move(in));
        for (int i = 0; i < ts; i++) {
            Layer o = layers.back();
            if (ops[i].type == OP_MAXPOOL || ops[i].type == OP_AVGPOOL) {
                o.H /= ops[i].kh;
                for (auto& w : o.W) w /= ops[i].kw;
            }
            layers.push_back(std::move(o));
        }
        meta32 = n;
        loff_at = prefix([&](int g) { return n[g]; }).off;
        for (Layer& l : layers) tabulate(l);
    }

    k::RaggedView view(size_t li) const {
        const Layer& l = layers[li];
        k::RaggedView v{};
        v.G = G; v.H = l.H;
        v.W = d32 + l.w; v.n = d32; v.poff = d64 + l.p;
        v.toff256 = d32 + l.t256.off; v.loff = d32 + loff_at;
        v.ntiles256 = l.t256.total; v.pixels = l.pixels;
        // patch shape for the 3x3 convs: the one that wastes fewer lanes on ragged right edges
        const bool use16 = l.H % 8 == 0 && (l.H % 4 != 0 || l.t16.total < l.t32.total);
        const Table &t2d = use16 ? l.t16 : l.t32, *flat = use16 ? l.f16 : l.f32;
        v.tw = use16 ? 16 : 32;
        v.toff2d = d32 + t2d.off; v.ntiles2d = t2d.total;
        v.toff2d_flat = d32 + flat[0].off; v.ntiles2d_flat = flat[0].total;
        v.toff2d_flat2 = d32 + flat[1].off; v.ntiles2d_flat2 = flat[1].total;
        const bool has32 = l.H % 4 == 0;
        v.toff2d_32 = d32 + l.t32.off; v.ntiles2d_32 = has32 ? l.t32.total : 0;
        v.toff2d_flat_32 = d32 + l.f32[0].off; v.ntiles2d_flat_32 = has32 ? l.f32[0].total : 0;
        v.toff2d_flat2_32 = d32 + l.f32[1].off; v.ntiles2d_flat2_32 = has32 ? l.f32[1].total : 0;
        v.toff2d_gap = d32 + l.gap.off;
        v.ntiles2d_gap = l.H % 8 == 0 ? l.gap.total : 0;
        v.max_w = 0;
        v.max_tile_px_ = 0;
        v.max_tile_px32_ = 0;
        v.min_w = INT32_MAX;
        for (int g = 0; g < G; g++) {
            const int64_t w = l.W[g], span = std::min<int64_t>(n[g], (v.tw - 1 + w - 1) / w + 1);
            v.max_tile_px_ = std::max(v.max_tile_px_, span * l.H * w);
            v.max_tile_px32_ = std::max(v.max_tile_px32_, std::min<int64_t>(n[g], (32 - 1 + w - 1) / w + 1) * l.H * w);
            v.min_w = std::min(v.min_w, (int)w);
            v.max_w = std::max(v.max_w, (int)w);
        }
        return v;
    }

private:
    // per-group counts -> their prefix table [G+1], appended to meta32
    template <class Count>
    Table prefix(Count count) {
        Table t{meta32.size(), 0};
        meta32.push_back(0);
        for (int g = 0; g < G; g++) { t.total += (int32_t)count(g); meta32.push_back(t.total); }
        return t;
    }
    void tabulate(Layer& l) {
        const int H = l.H;
        const std::vector<int32_t>& W = l.W;
        l.w = meta32.size();
        meta32.insert(meta32.end(), W.begin(), W.end());
        l.t256 = prefix([&](int g) { return ((int64_t)n[g] * H * W[g] + 255) / 256; });
        l.t32 = prefix([&](int g) { return n[g] * (H / 4) * ((W[g] + 31) / 32); });
        l.t16 = prefix([&](int g) { return n[g] * (H / 8) * ((W[g] + 15) / 16); });
        l.gap = prefix([&](int g) { return (H / 8) * (((int64_t)n[g] * ((W[g] + 2) & ~1) + 15) / 16); });
        for (int e = 0; e < 2; e++) {
            auto cols = [&, e](int g) { return (int64_t)n[g] * (e ? (W[g] + 1) & ~1 : W[g]); };
            l.f32[e] = prefix([&](int g) { return (H / 4) * ((cols(g) + 31) / 32); });
            l.f16[e] = prefix([&](int g) { return (H / 8) * ((cols(g) + 15) / 16); });
        }
        l.p = meta64.size();
        meta64.push_back(0);
        for (int g = 0; g < G; g++) { l.pixels += (int64_t)n[g] * H * W[g]; meta64.push_back(l.pixels); }
    }
};

}  // namespace ocrs
