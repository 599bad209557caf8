// Host-side plan of the detector, with no HIP in it (what sd_plan.h is for the extractor): the built-in YOLOv3 layer list, the shape pass
// of a network (yolo_plan_net: per-layer sizes, weight offsets, the kernel class of every convolution, FLOP totals), where the outputs of its
// [shortcut] and [route] layers live and which lists are refused (yolo_plan_storage) and THE choice of the kernel,
// tiles and grid that run a convolution at a batch size (yolo_plan_launch).  sd_yolo_api.hip launches what these records say and decides nothing
// itself; tests/test_yolo_plan.py compiles this header alone and pins the records.  The measurements behind the choices: DESIGN.md 4.1.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>
#include "sd_frontend.h"

// Tile sizes of the kernels the choice depends on (the kernels themselves: k_yolo.h)
#define SD_CV_BM 64          // k_conv_mfma: couts per workgroup
#define SD_CV_BN 256         // k_conv_mfma: pixels per workgroup
#define SD_C3_BM 128         // k_conv3x3_flat
#define SD_C3_BN 256
#define SD_C3_BK 32
#define SD_C3_MAXW 80
#define SD_G3_BM 128         // k_conv3x3_glds, k_conv_glds
#define SD_G3_BN 512
#define SD_B3F_MAXW 160      // k_conv3x3_b3: the widest map whose staged chunk fits its LDS
#define SD_B3C_MAXW 80       // k_conv3x3_b3c
// 1-D launch of the f32-class kernels: the pixel tiles rounded up to the 8 XCDs, times the filter tiles
#define SD_F32_GRID(tx, ty) (unsigned)((((tx) + 7) / 8) * 8 * (ty))

static const float kYoloV3Anchors[18] = {10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326};

// The layer list of src/yolo/yolov3.cfg (107 layers), restated programmatically.
static inline void yolo_v3_layers(std::vector<sd_yolo_layer>& L)
{
    auto conv = [&](int filters, int size, int stride, int bn = 1, int leaky = 1) {
        sd_yolo_layer l = {}; l.type = SD_YOLO_CONV; l.filters = filters; l.size = size; l.stride = stride; l.batch_normalize = bn; l.leaky = leaky;
        L.push_back(l);
    };
    auto shortcut = [&](int from) { sd_yolo_layer l = {}; l.type = SD_YOLO_SHORTCUT; l.from[0] = from; l.nfrom = 1; L.push_back(l); };
    auto route = [&](int a, int b = 0, int n = 1) { sd_yolo_layer l = {}; l.type = SD_YOLO_ROUTE; l.from[0] = a; l.from[1] = b; l.nfrom = n; L.push_back(l); };
    auto upsample = [&]() { sd_yolo_layer l = {}; l.type = SD_YOLO_UPSAMPLE; l.stride = 2; L.push_back(l); };
    auto yolo = [&](int m0, int m1, int m2) { sd_yolo_layer l = {}; l.type = SD_YOLO_YOLO; l.mask[0] = m0; l.mask[1] = m1; l.mask[2] = m2; L.push_back(l); };
    auto res = [&](int c, int n) { for (int i = 0; i < n; i++) { conv(c / 2, 1, 1); conv(c, 3, 1); shortcut(-3); } };
    conv(32, 3, 1);
    conv(64, 3, 2); res(64, 1);
    conv(128, 3, 2); res(128, 2);
    conv(256, 3, 2); res(256, 8);
    conv(512, 3, 2); res(512, 8);
    conv(1024, 3, 2); res(1024, 4);
    for (int i = 0; i < 3; i++) { conv(512, 1, 1); conv(1024, 3, 1); }
    conv(255, 1, 1, 0, 0); yolo(6, 7, 8);
    route(-4); conv(256, 1, 1); upsample(); route(-1, 61, 2);
    for (int i = 0; i < 3; i++) { conv(256, 1, 1); conv(512, 3, 1); }
    conv(255, 1, 1, 0, 0); yolo(3, 4, 5);
    route(-4); conv(128, 1, 1); upsample(); route(-1, 36, 2);
    for (int i = 0; i < 3; i++) { conv(128, 1, 1); conv(256, 3, 1); }
    conv(255, 1, 1, 0, 0); yolo(0, 1, 2);
}

static inline int yolo_resolve(int idx, int from) { return from < 0 ? idx + from : from; }

// The kernel family that computes a convolution; it also fixes the layout of the layer's weights (sd_yolo_load_darknet_weights).
enum SdYoloClass {
    SD_YC_NONE,        // not a convolution
    SD_YC_F16,         // k_yolo.h: f16 operands
    SD_YC_F32,         // k_yolo32.h: k_conv_f32
    SD_YC_WINO,        // k_yolo32w.h: Winograd F(2x2, 3x3), transformed weights at wOffW
    // k_yolo32b.h, three bf16 limbs per operand, split weights at wOffB (16-byte units):
    SD_YC_B3,          // k_conv_b3<2>, 128-filter tiles
    SD_YC_B3_64,       // k_conv_b3<1>, the 64-filter layers
    SD_YC_B3_FLAT,     // k_conv3x3_b3: 3 x 3 stride 1 on maps up to 160 wide, the nine taps share one staged chunk; weights walk [chunk][tap]
    SD_YC_B3_FLATC     // k_conv3x3_b3c: the same on maps up to 80 wide with 64-filter tiles and the weights staged per chunk too (wider maps do not fit its LDS)
};
static inline bool yolo_class_b3(int c) { return c >= SD_YC_B3; }
static inline bool yolo_class_b3_flat(int c) { return c == SD_YC_B3_FLAT || c == SD_YC_B3_FLATC; }
static inline int yolo_class_b3_wm(int c) { return c == SD_YC_B3_64 || c == SD_YC_B3_FLATC ? 1 : 2; }     // 64-filter wave rows per weight tile

struct SdYoloLayerPlan {
    int H = 0, W = 0, C = 0;           // output map and channels
    int cinPad = 0, coutPad = 0;       // convolutions: stored input channels; filters padded to the widest filter tile (weight / bias rows)
    int outC = 0;                      // stored channel count (255 -> 256)
    size_t wOff = 0, bOff = 0;
    int cls = SD_YC_NONE;
    size_t wOffW = 0, wOffB = 0;
};

struct SdYoloTotals {
    size_t wTotal = 0, bTotal = 0, wTotalW = 0, wTotalB = 0, vMax = 0;      // vMax: floats per image of the largest Winograd input transform
    int nconv = 0, totalRows = 0;
    double convFlops = 0;              // per image
    double mfmaFlops = 0;              // per image, as executed (Winograd layers: 16 multiplies per 2 x 2 block instead of 36)
    double mfmaFlopsBf16 = 0;          // per image: bf16 MFMA FLOPs executed by the limb kernels (six limb products per product)
};
struct SdYoloNetPlan : SdYoloTotals { std::vector<SdYoloLayerPlan> R; };

struct SdYoloPlanError { int code; const char* text; };      // code SD_OK: no error

// Shapes, offsets, kernel classes and FLOP totals of a network in one precision.
static inline SdYoloPlanError yolo_plan_net(const sd_yolo_layer* L, int n_layers, int net_w, int net_h, int classes, int precision, SdYoloNetPlan& P)
{
    P = SdYoloNetPlan();
    P.R.resize(n_layers);
    int H = net_h, W = net_w, C = 32;      // blob: 3 channels padded to 32
    for (int i = 0; i < n_layers; i++) {
        const sd_yolo_layer& l = L[i];
        SdYoloLayerPlan& r = P.R[i];
        if (l.type == SD_YOLO_CONV) {
            if ((l.size != 1 && l.size != 3) || (l.stride != 1 && l.stride != 2) || l.filters < 1) return {SD_ERR_UNSUPPORTED, "convolution size/stride not supported"};
            if (i == 0 && (l.size != 3 || l.stride != 1 || l.filters > 32)) return {SD_ERR_UNSUPPORTED, "first convolution must be 3x3, stride 1, <= 32 filters"};
            const int cinReal = i == 0 ? 3 : C;
            r.cinPad = i == 0 ? 32 : C;
            if (r.cinPad % 32) return {SD_ERR_UNSUPPORTED, "input channels must be a multiple of 32"};
            const int pad = l.size / 2;
            r.H = (H + 2 * pad - l.size) / l.stride + 1; r.W = (W + 2 * pad - l.size) / l.stride + 1; r.C = l.filters;
            r.outC = (l.filters + 31) / 32 * 32;
            r.coutPad = (l.filters + SD_G3_BM - 1) / SD_G3_BM * SD_G3_BM;
            r.wOff = P.wTotal; r.bOff = P.bTotal;
            P.wTotal += (size_t)r.coutPad * l.size * l.size * r.cinPad;
            P.bTotal += r.coutPad;
            const double flops = 2.0 * r.H * r.W * (double)l.filters * l.size * l.size * cinReal;
            P.convFlops += flops;
            r.cls = precision == SD_YOLO_F16 ? SD_YC_F16 : SD_YC_F32;
            // Winograd F(2x2, 3x3): 3 x 3, stride 1, >= 64 input channels (the fold runs once per cin channels) and whole 128-filter tiles
            if (precision == SD_YOLO_F32W && i > 0 && l.size == 3 && l.stride == 1 && r.cinPad >= 64 && (r.cinPad % 16) == 0 && l.filters >= 128 && (l.filters % 128) == 0) {
                const size_t blocks = (size_t)((r.H + 1) / 2) * ((r.W + 1) / 2);
                r.cls = SD_YC_WINO;
                r.wOffW = P.wTotalW; P.wTotalW += (size_t)r.coutPad * 16 * r.cinPad;
                P.vMax = std::max(P.vMax, blocks * 16 * r.cinPad);
                P.mfmaFlops += 2.0 * blocks * 16.0 * (double)l.filters * cinReal;
            } else if (precision == SD_YOLO_F32X3 && i > 0 && l.filters >= 64 && (l.filters > 64 || (l.filters % 64) == 0) && (r.cinPad % 16) == 0) {
                // three bf16 limbs per operand: the layers k_conv_f32 runs on 128-filter tiles, and the 64-filter ones
                const bool flat = l.size == 3 && l.stride == 1 && r.W <= SD_B3F_MAXW && l.filters > 64;
                r.cls = flat ? (r.W <= SD_B3C_MAXW ? SD_YC_B3_FLATC : SD_YC_B3_FLAT) : (l.filters == 64 ? SD_YC_B3_64 : SD_YC_B3);
                r.wOffB = P.wTotalB; P.wTotalB += (size_t)(r.coutPad / 128) * (l.size * l.size * (r.cinPad / 16)) * 2 * 6 * 64;      // 16-byte fragments
                P.mfmaFlopsBf16 += 6 * flops;
            } else P.mfmaFlops += flops;
            P.nconv++;
        } else if (l.type == SD_YOLO_SHORTCUT) {
            const int f = yolo_resolve(i, l.from[0]);
            if (f < 0 || f >= i || P.R[f].H != H || P.R[f].W != W || P.R[f].C != C) return {SD_ERR_INVALID, "bad shortcut"};
            r.H = H; r.W = W; r.C = C; r.outC = C;
        } else if (l.type == SD_YOLO_ROUTE) {
            const int f0 = yolo_resolve(i, l.from[0]);
            if (f0 < 0 || f0 >= i) return {SD_ERR_INVALID, "bad route"};
            r.H = P.R[f0].H; r.W = P.R[f0].W; r.C = P.R[f0].C;
            if (l.nfrom == 2) {
                const int f1 = yolo_resolve(i, l.from[1]);
                if (f1 < 0 || f1 >= i || P.R[f1].H != r.H || P.R[f1].W != r.W) return {SD_ERR_INVALID, "bad route"};
                r.C += P.R[f1].C;
            }
            r.outC = r.C;
        } else if (l.type == SD_YOLO_UPSAMPLE) {
            r.H = 2 * H; r.W = 2 * W; r.C = C; r.outC = C;
        } else if (l.type == SD_YOLO_YOLO) {
            if (C != 3 * (5 + classes)) return {SD_ERR_INVALID, "[yolo] input must have 3*(5+classes) channels"};
            r.H = H; r.W = W; r.C = C; r.outC = C;
            P.totalRows += H * W * 3;
        } else return {SD_ERR_INVALID, "unknown layer type"};
        H = r.H; W = r.W; C = r.C;
        if ((l.type == SD_YOLO_CONV) && (r.C % 4) && r.C != 3 * (5 + classes)) return {SD_ERR_UNSUPPORTED, "filters must be a multiple of 4"};
    }
    return {SD_OK, nullptr};
}

// Where the outputs of the layers that compute nothing live, decided at creation: which [shortcut]s are fused into the epilogue of the convolution
// before them, and which 2-input [route]s get their second input written IN PLACE by its producer (f32-class modes: only the up-sampled half is
// then copied, k_upsample_into_f32) instead of being copied whole (k_upsample_concat).  Every list the forward pass could not run is refused here,
// before anything is allocated or launched: sd_yolo_create_prec creates no detector for it.
struct SdYoloStorage { std::vector<char> fused, inPlace; };      // per layer: fused [shortcut]; 2-input [route] whose second input is written in place
static inline SdYoloPlanError yolo_plan_storage(const sd_yolo_layer* L, int n_layers, const SdYoloNetPlan& P, bool f32, SdYoloStorage& S)
{
    S.fused.assign(n_layers, 0); S.inPlace.assign(n_layers, 0);
    std::vector<char> strided(n_layers, 0);      // tensors written in place into a route's buffer: their channel stride is the route's
    auto read_by_route = [&](int layer, int except) {
        for (int j = 0; j < n_layers; j++)
            if (j != except && L[j].type == SD_YOLO_ROUTE)
                for (int k = 0; k < L[j].nfrom; k++) if (yolo_resolve(j, L[j].from[k]) == layer) return true;
        return false;
    };
    for (int i = 0; i < n_layers; i++) {
        const sd_yolo_layer& l = L[i];
        if (l.type == SD_YOLO_SHORTCUT) {
            // fused when the preceding convolution's output has no other consumer (the layer after a [shortcut] reads the sum, never the addend)
            bool fuse = i > 0 && L[i - 1].type == SD_YOLO_CONV && yolo_resolve(i, l.from[0]) != i - 1;
            for (int j = 0; fuse && j < n_layers; j++) {
                if (j == i) continue;
                if (L[j].type == SD_YOLO_SHORTCUT || L[j].type == SD_YOLO_ROUTE)
                    for (int k = 0; k < L[j].nfrom; k++) if (yolo_resolve(j, L[j].from[k]) == i - 1) fuse = false;
            }
            if (!fuse) return {SD_ERR_UNSUPPORTED, "unfused [shortcut] is not implemented: it must follow a convolution whose output nothing else reads"};
            const int f = yolo_resolve(i, l.from[0]);
            if (L[f].type == SD_YOLO_UPSAMPLE) return {SD_ERR_UNSUPPORTED, "[shortcut] from an [upsample]: it is materialised only inside a [route]"};
            S.fused[i] = 1;
        } else if (l.type == SD_YOLO_UPSAMPLE) {
            // materialised only inside the following 2-input route; stand-alone upsample unsupported
            if (!(i >= 1 && i + 1 < n_layers && L[i + 1].type == SD_YOLO_ROUTE && L[i + 1].nfrom == 2 && yolo_resolve(i + 1, L[i + 1].from[0]) == i))
                return {SD_ERR_UNSUPPORTED, "[upsample] must feed a 2-input [route] as its first input"};
            if (L[i - 1].type == SD_YOLO_UPSAMPLE) return {SD_ERR_UNSUPPORTED, "[upsample] of an [upsample]"};
            if (read_by_route(i, i + 1)) return {SD_ERR_UNSUPPORTED, "[upsample] must feed a 2-input [route] as its first input"};
        } else if (l.type == SD_YOLO_ROUTE) {
            if (l.nfrom != 1 && l.nfrom != 2) return {SD_ERR_INVALID, "bad route"};
            const int fa = yolo_resolve(i, l.from[0]);
            if (l.nfrom == 1) {
                if (L[fa].type == SD_YOLO_UPSAMPLE) return {SD_ERR_UNSUPPORTED, "[upsample] must feed a 2-input [route] as its first input"};
                continue;
            }
            const int fb = yolo_resolve(i, l.from[1]);
            if (L[fa].type != SD_YOLO_UPSAMPLE || fa != i - 1 || L[fb].type == SD_YOLO_UPSAMPLE)
                return {SD_ERR_UNSUPPORTED, "a 2-input [route] must take the [upsample] before it as its first input"};
        }
    }
    // in place (f32-class modes): the producer is a convolution (with or without a fused shortcut), its tensor is dense, and one route only may
    // own the tensor's storage
    for (int i = 0; f32 && i < n_layers; i++) {
        const sd_yolo_layer& l = L[i];
        if (l.type != SD_YOLO_ROUTE || l.nfrom != 2) continue;
        const int fb = yolo_resolve(i, l.from[1]), src = yolo_resolve(i, l.from[0]) - 1;      // src: the layer the [upsample] reads
        const SdYoloLayerPlan& ra = P.R[src]; const SdYoloLayerPlan& rb = P.R[fb];
        const int conv = L[fb].type == SD_YOLO_CONV ? fb : (L[fb].type == SD_YOLO_SHORTCUT && S.fused[fb] ? fb - 1 : -1);
        if (conv >= 0 && rb.outC == rb.C && P.R[conv].outC == P.R[conv].C && (ra.C % 4) == 0 && (rb.C % 4) == 0 && !read_by_route(fb, i)) {
            S.inPlace[i] = 1; strided[conv] = strided[fb] = 1;
        }
    }
    // every other 2-input route is copied whole: k_upsample_concat moves 16-byte pieces of dense tensors
    for (int i = 0; i < n_layers; i++) {
        const sd_yolo_layer& l = L[i];
        if (l.type != SD_YOLO_ROUTE || l.nfrom != 2 || S.inPlace[i]) continue;
        const int fb = yolo_resolve(i, l.from[1]), src = yolo_resolve(i, l.from[0]) - 1;
        const SdYoloLayerPlan& ra = P.R[src]; const SdYoloLayerPlan& rb = P.R[fb];
        const int piece = f32 ? 4 : 8;
        if (ra.outC != ra.C || rb.outC != rb.C || strided[src] || strided[fb] || (ra.C % piece) || (rb.C % piece))
            return {SD_ERR_UNSUPPORTED, f32 ? "route inputs must be dense, channels % 4 == 0" : "route inputs must be dense, channels % 8 == 0"};
    }
    return {SD_OK, nullptr};
}

// Every kernel instantiation a convolution can run on, the f16 mode's first: X(id, workgroup size, the kernel as sd_yolo_api.hip knows it).
// The only list that names them: the enum, the names a kernel trace shows and sd_yolo_api.hip's function table all expand it.
#define SD_YOLO_KERNELS(X) \
    X(CONV_FIRST, 256, k_conv_first) \
    X(GLDS_8_1, 512, k_conv_glds<8, 1>) \
    X(GLDS_4_1, 256, k_conv_glds<4, 1>) \
    X(GLDS_8_3, 512, k_conv_glds<8, 3>) \
    X(GLDS_4_3, 256, k_conv_glds<4, 3>) \
    X(G3_80, 512, k_conv3x3_glds<80>) \
    X(G3_160, 512, k_conv3x3_glds<160>) \
    X(C3_FLAT, 256, k_conv3x3_flat) \
    X(MFMA_64, 256, k_conv_mfma<64>) \
    X(MFMA_32, 256, k_conv_mfma<32>) \
    X(F32_8_1_1_8, 512, k_conv_f32<8, 1, 1, 8>) \
    X(F32_16_1_1_4, 256, k_conv_f32<16, 1, 1, 4>) \
    X(F32_16_1_2_4, 256, k_conv_f32<16, 1, 2, 4>) \
    X(F32_16_2_2_4, 256, k_conv_f32<16, 2, 2, 4>) \
    X(WINO_16_2, 256, k_wino_gemm_f32<16, 2>) \
    X(B3_1, 256, k_conv_b3<1>) \
    X(B3_2, 256, k_conv_b3<2>) \
    X(B3F_3, 256, k_conv3x3_b3<3, 2, 2>) \
    X(B3F_4, 256, k_conv3x3_b3<4, 2, 2>) \
    X(B3F_5, 256, k_conv3x3_b3<5, 2, 2>) \
    X(B3F_8, 256, k_conv3x3_b3<8, 2, 2>) \
    X(B3C_5, 512, k_conv3x3_b3c<5>) \
    X(B3C_6, 512, k_conv3x3_b3c<6>)
enum SdYoloKernel {
#define X(id, block, ...) SD_YK_##id,
    SD_YOLO_KERNELS(X)
#undef X
    SD_YK_COUNT, SD_YK_F32_FIRST = SD_YK_F32_8_1_1_8
};
static const struct { const char* name; int block; } kYoloKernelInfo[SD_YK_COUNT] = {
#define X(id, block, ...) {#__VA_ARGS__, block},
    SD_YOLO_KERNELS(X)
#undef X
};

struct SdYoloLaunch {
    int kernel = 0;                          // SdYoloKernel
    unsigned gridX = 1, gridY = 1;
    int block = 0;
    int tilesX = 0, tilesY = 0, groupY = 0;  // f32-class kernels: pixel tiles, filter tiles, filter tiles walked back to back on a pixel tile
    int width = 0;                           // k_conv3x3_b3 / k_conv3x3_b3c: the map width that sizes their dynamic LDS
    unsigned inputGrid = 0;                  // Winograd layers: workgroups of k_wino_input ahead of the GEMM
};

// filter tiles walked back to back on a pixel tile (k_conv_f32's workgroup order): the largest power of two that divides tilesY and
// keeps the group's weights (bm filters x kdim floats per tile) within 2.5 MB of an XCD's 4 MB L2
static inline int f32_group_y(int tilesY, int bm, int kdim)
{
    int g = 1;
    while (2 * g <= tilesY && tilesY % (2 * g) == 0 && (size_t)(2 * g) * bm * kdim * 4 <= (size_t)2560 * 1024) g *= 2;
    return g;
}

// Division by a number known on the host, for the kernels: n / d == (mulhi32(n, m) + n) >> s for every n < 2^31 (the sum then fits 32 bits),
// with s = ceil(log2 d) and m = ceil(2^(32 + s) / d) - 2^32 (Granlund & Montgomery 1994: 2^(32 + s) <= (m + 2^32) d <= 2^(32 + s) + 2^s).
// d = 1 and the powers of two come out as m = 0.  tests/test_conv_f32_magic_div.py walks the full ranges the detector divides.
struct SdMagic { unsigned m, s; };
static inline SdMagic sd_magic_div(unsigned d)
{
    unsigned s = 0;
    while ((1ull << s) < d) s++;
    return {(unsigned)((((1ull << (32 + s)) + d - 1) / d) - (1ull << 32)), s};
}
static inline unsigned sd_magic_quot(unsigned n, SdMagic k) { return ((unsigned)(((unsigned long long)n * k.m) >> 32) + n) >> k.s; }

// What k_conv_f32's set-up takes from the host (SdConvArgsF, k_yolo32.h): the four divisors of its pixel split and workgroup order, and the byte
// distances its gather pointers move by at a tap change -- to the next column, and from a filter row's last column to the next row's first (negative
// on maps narrower than the filter).  `W`: the INPUT map's width.
struct SdF32Setup { SdMagic hoWo, wo, perGroup, groupY; long long tapCol, tapRow; };
static inline SdF32Setup yolo_f32_setup(int tilesX, int groupY, int Ho, int Wo, int W, int ksize, int cinStride)
{
    SdF32Setup S;
    S.hoWo = sd_magic_div((unsigned)(Ho * Wo)); S.wo = sd_magic_div((unsigned)Wo);
    S.perGroup = sd_magic_div((unsigned)(((tilesX + 7) / 8) * groupY)); S.groupY = sd_magic_div((unsigned)groupY);
    S.tapCol = 4ll * cinStride; S.tapRow = 4ll * (W - ksize + 1) * cinStride;
    return S;
}

// The scalar staging walk of k_conv_f32's two unconditional tiles (128 and 64 filters; k_yolo32.h, "The scalar walk"): a staging load's address is
// descriptor base + per-lane byte offset (32 bits, fixed for the tile) + one scalar byte offset per descriptor that walks the K steps.
//   SD_F32_WALK_RECORDS    record count of the activations' descriptor: its base, the tile's anchor, is tap (0, 0), channel 0 of the tile's first
//                          pixel and every live lane's offset + walk + 16 stays below it (yolo_f32_walk_fits)
//   SD_F32_WALK_SENTINEL   the per-lane offset of a padded tap (and of a pixel beyond the last): outside the records whatever the scalar offset adds,
//                          so the descriptor's range check answers zeros without touching memory
#define SD_F32_WALK_RECORDS 0x80000000u
#define SD_F32_WALK_SENTINEL 0x80000000u
// Does a layer fit that walk?  A tile of bn output pixels spans at most (bn - 1) / (Ho Wo) + 1 image boundaries, and within an image a pixel's
// tap (0, 0) lies less than H W input pixels behind another's: a live lane's offset is below ((bn - 1) / (Ho Wo) + 2) H W pixels + its piece (48
// bytes); the walk adds at most the last tap's distance ((ksize - 1) (W + 1) pixels) and the tap's cin channels.  tests/cpp/conv_f32_offsets_check.cpp
// walks every lane of the detector's layers against it.
static inline bool yolo_f32_walk_fits(int bn, int H, int W, int Ho, int Wo, int ksize, int cin, int cinStride)
{
    const long long lane = ((long long)((bn - 1) / (Ho * Wo)) + 2) * H * W * 4ll * cinStride + 48;
    const long long walk = (long long)(ksize - 1) * (W + 1) * 4ll * cinStride + 4ll * cin;
    return lane + walk + 16 <= (long long)SD_F32_WALK_RECORDS;
}

// The launch of convolution `l` (the network's first when `first`) with shape record `r` on a batch of n images.
static inline SdYoloLaunch yolo_plan_launch(const sd_yolo_layer& l, const SdYoloLayerPlan& r, bool first, int n)
{
    SdYoloLaunch K;
    const int npix = n * r.H * r.W, taps = l.size * l.size;
    const bool s3 = l.size == 3 && l.stride == 1;      // the input map then has the output's width
    auto tiles = [&](SdYoloKernel k, int bn, int tilesY, int groupY) {
        K.kernel = k; K.tilesX = (npix + bn - 1) / bn; K.tilesY = tilesY; K.groupY = groupY; K.gridX = SD_F32_GRID(K.tilesX, K.tilesY);
    };
    auto grid2 = [&](SdYoloKernel k, int bn, int gridY) { K.kernel = k; K.gridX = (npix + bn - 1) / bn; K.gridY = gridY; };
    switch (r.cls) {
    case SD_YC_F16: {
        const bool flat3 = s3 && r.W <= 160 && l.filters % SD_G3_BM == 0 && r.cinPad % 32 == 0 && npix >= SD_G3_BN;
        if (first) { K.kernel = SD_YK_CONV_FIRST; K.gridX = (unsigned)(((size_t)n * r.H * r.W + 255) / 256); }
        else if (!flat3 && r.cinPad % 32 == 0 && npix >= 512 && (l.size == 1 || l.filters >= SD_G3_BM / 2)) {
            const int ct = r.coutPad / SD_G3_BM;
            const bool big = ((npix + 511) / 512) * ct >= 256;      // else 256-pixel tiles on 4 waves, two workgroups per CU
            if (l.size == 1) grid2(big ? SD_YK_GLDS_8_1 : SD_YK_GLDS_4_1, big ? 512 : 256, ct);
            else grid2(big ? SD_YK_GLDS_8_3 : SD_YK_GLDS_4_3, big ? 512 : 256, ct);
        } else if (flat3) grid2(r.W <= 80 ? SD_YK_G3_80 : SD_YK_G3_160, SD_G3_BN, l.filters / SD_G3_BM);
        else if (s3 && r.W <= SD_C3_MAXW && l.filters % SD_C3_BM == 0 && r.cinPad % SD_C3_BK == 0) grid2(SD_YK_C3_FLAT, SD_C3_BN, l.filters / SD_C3_BM);
        else grid2(r.cinPad % 64 == 0 ? SD_YK_MFMA_64 : SD_YK_MFMA_32, SD_CV_BN, (l.filters + SD_CV_BM - 1) / SD_CV_BM);
        break;
    }
    case SD_YC_F32: {
        // 128-filter layers: 128 x 128 tiles on 4 waves with 16-channel K steps, three workgroups per CU; the <= 64- / <= 32-filter layers, which
        // would waste half or three quarters of such a tile: 64 x 256 and 32 x 256; the first layer (3 -> 8 input channels): 32 x 512 on 8 waves
        const int kdim = (first ? 8 : r.cinPad) * taps;
        if (first) tiles(SD_YK_F32_8_1_1_8, 512, (l.filters + 31) / 32, f32_group_y((l.filters + 31) / 32, 32, kdim));
        else if (l.filters <= 32) tiles(SD_YK_F32_16_1_1_4, 256, 1, 1);
        else if (l.filters <= 64) tiles(SD_YK_F32_16_1_2_4, 256, 1, 1);
        else tiles(SD_YK_F32_16_2_2_4, 128, r.coutPad / 128, f32_group_y(r.coutPad / 128, 128, kdim));
        break;
    }
    case SD_YC_WINO: {
        // 128 filters x 64 blocks per workgroup, ALL filter tiles back to back on a block tile: V is the big operand here
        const size_t nblk = (size_t)n * ((r.H + 1) / 2) * ((r.W + 1) / 2);
        K.kernel = SD_YK_WINO_16_2; K.tilesX = (int)((nblk + 63) / 64); K.tilesY = r.coutPad / 128; K.groupY = K.tilesY;
        K.gridX = SD_F32_GRID(K.tilesX, K.tilesY);
        K.inputGrid = (unsigned)std::min<size_t>((nblk * (r.cinPad / 4) + 255) / 256, 65536);
        break;
    }
    case SD_YC_B3: tiles(SD_YK_B3_2, 128, r.coutPad / 128, f32_group_y(r.coutPad / 128, 128, r.cinPad * taps * 3 / 2)); break;
    case SD_YC_B3_64: tiles(SD_YK_B3_1, 256, 1, 1); break;
    case SD_YC_B3_FLAT: {
        const int np = (4 * (128 + 2 * r.W + 2) + 255) / 256;      // 16-byte pieces of a staged chunk per thread
        tiles(np <= 3 ? SD_YK_B3F_3 : np == 4 ? SD_YK_B3F_4 : np == 5 ? SD_YK_B3F_5 : SD_YK_B3F_8, 128, r.coutPad / 128, f32_group_y(r.coutPad / 128, 128, r.cinPad * taps * 3 / 2));
        K.width = r.W;
        break;
    }
    case SD_YC_B3_FLATC: {
        const int np = (4 * (512 + 2 * r.W + 2) + 511) / 512;
        tiles(np <= 5 ? SD_YK_B3C_5 : SD_YK_B3C_6, 512, r.coutPad / 64, f32_group_y(r.coutPad / 64, 64, r.cinPad * 9 * 3 / 2));
        K.gridX = 8 * (unsigned)std::min(((K.tilesX + 7) / 8) * K.tilesY, 32);      // persistent: one workgroup per CU, 32 per XCD
        K.width = r.W;
        break;
    }
    default: break;
    }
    K.block = kYoloKernelInfo[K.kernel].block;
    return K;
}
