// The detector part of the C ABI (include/sd_frontend.h, sd_yolo_*): its own translation unit, so that a change to a front-end kernel
// does not recompile the convolution stack and vice versa.  Kernels: k_yolo.h (f16 mode), k_yolo32.h / k_yolo32w.h / k_yolo32b.h (f32-class modes).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <climits>
#include <cmath>
#include <string>
#include <memory>
#include <vector>
#include "sd_common.h"
#include "sd_yolo.h"

template <typename T>      // the region layer of a head (its input: layer i - 1), T = float | _Float16
static void yolo_decode(const sd_yolo* y, const sd_yolo_layer& l, const sd_yolo::Rt& r, int n, float conf_threshold, int rowBase, hipStream_t s)
{
    const float* an = y->anchors;
    const int rows = n * r.H * r.W * 3;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_region_decode<T>), dim3((rows + 255) / 256), dim3(256), 0, s, r.as<const T>(), r.outC, r.H, r.W, n, an[2 * l.mask[0]],
                       an[2 * l.mask[0] + 1], an[2 * l.mask[1]], an[2 * l.mask[1] + 1], an[2 * l.mask[2]], an[2 * l.mask[2] + 1],
                       y->netW, y->netH, conf_threshold, rowBase, y->d_dets, y->d_ndet, y->detCap, n == 1 ? y->d_raw : nullptr);
}

extern "C" {

// ---------------------------------------------------------------- detector (YOLOv3 on MFMA)
int sd_yolo_v3_layers(sd_yolo_layer* layers, int cap, int* n, float anchors[18])
{
    if (!n) return SD_ERR_INVALID;
    std::vector<sd_yolo_layer> L;
    yolo_v3_layers(L);
    *n = (int)L.size();
    if (anchors) memcpy(anchors, kYoloV3Anchors, sizeof(kYoloV3Anchors));
    if (layers) {
        if (cap < (int)L.size()) return set_err(SD_ERR_CAPACITY, "layer buffer too small");
        memcpy(layers, L.data(), L.size() * sizeof(sd_yolo_layer));
    }
    return SD_OK;
}

// The functions of sd_yolo_plan.h's kernel list, by kernel id
static const void* const kYoloKernelFn[SD_YK_COUNT] = {
#define X(id, block, ...) (const void*)__VA_ARGS__,
    SD_YOLO_KERNELS(X)
#undef X
};

// Dynamic LDS of kernel k, from the kernel headers' macros; only k_conv3x3_b3 / k_conv3x3_b3c size theirs by the map width
static int yolo_kernel_lds(int k, int width)
{
    switch (k) {
    case SD_YK_GLDS_8_1: case SD_YK_GLDS_8_3: return 3 * (512 * 64 + SD_G3_WBYTES);
    case SD_YK_GLDS_4_1: case SD_YK_GLDS_4_3: return 3 * (256 * 64 + SD_G3_WBYTES);
    case SD_YK_G3_80: return SD_G3_LDS(80);
    case SD_YK_G3_160: return SD_G3_LDS(160);
    case SD_YK_F32_8_1_1_8: return SD_F32_LDS(8, 1, 1, 8);
    case SD_YK_F32_16_1_1_4: return SD_F32_LDS(16, 1, 1, 4);
    case SD_YK_F32_16_1_2_4: return SD_F32_LDS(16, 1, 2, 4);
    case SD_YK_F32_16_2_2_4: return SD_F32_LDS(16, 2, 2, 4);
    case SD_YK_WINO_16_2: return SD_WINO_LDS(16, 2);
    case SD_YK_B3_1: return SD_B3_LDS(1);
    case SD_YK_B3_2: return SD_B3_LDS(2);
    case SD_YK_B3F_3: case SD_YK_B3F_4: case SD_YK_B3F_5: case SD_YK_B3F_8: return SD_B3F_LDS(width, 128);
    case SD_YK_B3C_5: case SD_YK_B3C_6: return SD_B3C_LDS(width);
    default: return 0;      // static LDS only
    }
}

// Launches what a launch record says; `args`: the addresses of the kernel's arguments
static int yolo_launch(const SdYoloLaunch& K, void** args, hipStream_t s)
{
    (void)hipLaunchKernel(kYoloKernelFn[K.kernel], dim3(K.gridX, K.gridY), dim3(K.block), args, (size_t)yolo_kernel_lds(K.kernel, K.width), s);
    LAUNCH_CHECK(kYoloKernelInfo[K.kernel].name);
    return SD_OK;
}

// The dynamic-LDS limits of the kernels the detector's mode launches, raised once at creation (for the widest map the plan gives a kernel)
static int yolo_raise_lds_limits(const sd_yolo* y)
{
    for (int k = y->f32 ? SD_YK_F32_FIRST : 0; k < (y->f32 ? SD_YK_COUNT : SD_YK_F32_FIRST); k++)
        HIPCHK(sd_raise_lds_limit(kYoloKernelFn[k], yolo_kernel_lds(k, k >= SD_YK_B3C_5 ? SD_B3C_MAXW : SD_B3F_MAXW)));
    HIPCHK(sd_raise_lds_limit((const void*)k_yolo_nms, SD_NMS_LDS));
    return SD_OK;
}

int sd_yolo_create(sd_yolo** out, const sd_yolo_layer* layers, int n_layers, const float anchors[18], int classes, int net_w,
                   int net_h, int max_batch)
{
    return sd_yolo_create_prec(out, layers, n_layers, anchors, classes, net_w, net_h, max_batch, SD_YOLO_F16);
}

int sd_yolo_create_prec(sd_yolo** out, const sd_yolo_layer* layers, int n_layers, const float anchors[18], int classes, int net_w,
                        int net_h, int max_batch, int precision)
{
    if (!out) return SD_ERR_INVALID;
    *out = nullptr;
    if (precision != SD_YOLO_F16 && precision != SD_YOLO_F32 && precision != SD_YOLO_F32W && precision != SD_YOLO_F32X3)
        return set_err(SD_ERR_INVALID, "precision must be SD_YOLO_F16, SD_YOLO_F32, SD_YOLO_F32W or SD_YOLO_F32X3");
    if (!layers || n_layers < 1 || !anchors || classes != 80 || net_w < 32 || net_h < 32 || (net_w % 32) || (net_h % 32) || max_batch < 1)
        return set_err(SD_ERR_INVALID, "bad detector arguments (classes must be 80, net size a multiple of 32)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_err(SD_ERR_NO_DEVICE, "no HIP device: the detector has no CPU fallback");
    std::unique_ptr<sd_yolo> y(new sd_yolo());
    SdYoloNetPlan P;
    const SdYoloPlanError pe = yolo_plan_net(layers, n_layers, net_w, net_h, classes, precision, P);
    if (pe.code != SD_OK) return set_err(pe.code, pe.text);
    const bool f32mode = precision != SD_YOLO_F16;
    SdYoloStorage S;                                      // fused shortcuts, in-place routes -- and the refusal of every list the forward could not run
    const SdYoloPlanError se = yolo_plan_storage(layers, n_layers, P, f32mode, S);
    if (se.code != SD_OK) return set_err(se.code, se.text);
    (SdYoloTotals&)*y = P;
    y->L.assign(layers, layers + n_layers);
    y->R.assign(P.R.begin(), P.R.end());
    y->netW = net_w; y->netH = net_h; y->classes = classes; y->maxBatch = max_batch;
    y->f32 = precision == SD_YOLO_F32 || precision == SD_YOLO_F32W || precision == SD_YOLO_F32X3;
    y->wino = precision == SD_YOLO_F32W;
    y->b3 = precision == SD_YOLO_F32X3;
    const size_t eb = y->f32 ? 4 : 2;                     // bytes per activation element
    memcpy(y->anchors, anchors, sizeof(y->anchors));
    y->detCap = 8192;
    // ---- device memory
    bool ok = true;
    auto alloc = [&](auto& buf, size_t bytes) { ok = ok && buf.alloc(bytes) == hipSuccess; };
    const size_t nB = (size_t)max_batch;
    if (y->f32) alloc(y->d_blob8, nB * net_h * net_w * 8 * 4);
    else alloc(y->d_blob4, nB * net_h * net_w * 4 * 2);
    alloc(y->d_zero, 256);
    if (ok) ok = hipMemset(y->d_zero, 0, 256) == hipSuccess;

    if (!y->f32) {
        alloc(y->d_wgt, y->wTotal * 2 + 64);                        // f16 weights: the f16 mode only
    } else {
        alloc(y->d_wgt32, y->wTotal * 4 + 64);
        if (y->wTotalW) { alloc(y->d_wgtW, y->wTotalW * 4 + 64); alloc(y->d_V, nB * y->vMax * 4 + 64); }
        if (y->wTotalB) alloc(y->d_wgtB, y->wTotalB * 16 + 65536);  // slack: the kernels request weight fragments up to two steps past a tile's last
    }
    alloc(y->d_bias, y->bTotal * 4 + 64);
    alloc(y->d_dets, nB * y->detCap * sizeof(SdDet));
    alloc(y->d_ndet, nB * 4);
    alloc(y->d_raw, (size_t)y->totalRows * (5 + classes) * 4 + 64);
    alloc(y->d_ct, 8 * 8192);
    alloc(y->d_rt, 8 * 8192);
    for (int i = 0; ok && i < n_layers; i++) {
        const sd_yolo_layer& l = y->L[i];
        sd_yolo::Rt& r = y->R[i];
        if (l.type == SD_YOLO_CONV) {
            alloc(r.own, nB * r.H * r.W * r.outC * eb + 64);
            r.out = r.own;
            if (ok && r.outC != r.C) ok = hipMemset(r.out, 0, nB * r.H * r.W * r.outC * eb) == hipSuccess;
        } else if (l.type == SD_YOLO_SHORTCUT) {
            // fused into the preceding convolution's epilogue (yolo_plan_storage refuses the lists where that output has another consumer)
            r.out = y->R[i - 1].out; r.alias = true;
        } else if (l.type == SD_YOLO_ROUTE && l.nfrom == 1) {
            r.out = y->R[yolo_resolve(i, l.from[0])].out; r.alias = true; r.outC = y->R[yolo_resolve(i, l.from[0])].outC;
        } else if (l.type == SD_YOLO_ROUTE) {
            alloc(r.own, nB * r.H * r.W * r.outC * eb + 64);
            r.out = r.own;
        } else if (l.type == SD_YOLO_UPSAMPLE) {
            // materialised only inside the following 2-input route (yolo_plan_storage has checked that one follows)
        } else if (l.type == SD_YOLO_YOLO) {
            r.out = y->R[i - 1].out; r.alias = true; r.outC = y->R[i - 1].outC;
        }
    }
    // f32-class modes: the second input of a 2-input [route] (yolov3.cfg: layers 61 and 36, the skip connections of the two up-sampling branches) is
    // written IN PLACE -- its producer's output pointer becomes the route buffer at the channel offset, its stride the route's channel count -- so the
    // route copies only the up-sampled half (k_upsample_into_f32).  Possible when the producer is a convolution (with or without a fused shortcut)
    // and its tensor is dense; every consumer reads it through (pointer, channel stride) anyway.
    for (int i = 0; ok && i < n_layers; i++) {
        if (!S.inPlace[i]) continue;                       // yolo_plan_storage: the producer is a convolution (with or without a fused shortcut), its tensor dense, this route its only one
        const sd_yolo_layer& l = y->L[i];
        const int fa = yolo_resolve(i, l.from[0]), fb = yolo_resolve(i, l.from[1]);
        const int src = yolo_resolve(fa, -1);
        sd_yolo::Rt& rb = y->R[fb];
        const int conv = y->L[fb].type == SD_YOLO_CONV ? fb : fb - 1;
        float* at = y->R[i].as<float>() + y->R[src].C;
        y->R[conv].out = at; y->R[conv].outC = y->R[i].C;
        rb.out = at; rb.outC = y->R[i].C;
        y->R[i].alias = true;                              // marks the route: its second input is already in place
    }
    if (ok) ok = hipStreamCreateWithFlags(&y->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) return set_err(SD_ERR_HIP, "detector allocation failed");
    const int rc = yolo_raise_lds_limits(y.get());
    if (rc == SD_OK) *out = y.release();
    return rc;
}

// Overlap mode (f32-class modes): blobFromImage runs on an internal stream ahead of the pass's first convolution, the three region decodes on
// another one behind their heads' convolutions, ordered by events; sd_yolo_boxes_device (on ITS stream argument) waits for the decodes.  With
// the next pass already enqueued on the convolution stream, its convolutions start while this pass's decode / NMS / download run beside them.
// The stream given to sd_yolo_forward_device then is NOT a completion point for the decoded rows: consume them through sd_yolo_boxes_device /
// sd_yolo_boxes_batch (any stream) or the host forms (they synchronise the device).
int sd_yolo_set_overlap(sd_yolo* y, int on)
{
    if (!y) return SD_ERR_INVALID;
    if (on && !y->f32) return set_err(SD_ERR_UNSUPPORTED, "overlap mode exists for the f32-class detector modes");
    int heads = 0;
    for (const sd_yolo_layer& l : y->L) heads += l.type == SD_YOLO_YOLO;
    if (on && heads > 3) return set_err(SD_ERR_UNSUPPORTED, "overlap mode orders at most three [yolo] heads");
    if (on && !y->sPre) {
        HIPCHK(hipStreamCreateWithFlags(&y->sPre, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&y->sPost, hipStreamNonBlocking));
        hipEvent_t* evs[] = {&y->evBlob, &y->evL0, &y->evHead[0], &y->evHead[1], &y->evHead[2], &y->evDecoded, &y->evNms};
        for (hipEvent_t* e : evs) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    if (!on && y->overlap) HIPCHK(hipDeviceSynchronize());
    y->overlap = on != 0;
    return SD_OK;
}

int sd_yolo_destroy(sd_yolo* y) { if (y) { (void)hipDeviceSynchronize(); delete y; } return SD_OK; }

int sd_yolo_weight_count(const sd_yolo* y, size_t* n_floats)
{
    if (!y || !n_floats) return SD_ERR_INVALID;
    size_t n = 0;
    for (size_t i = 0; i < y->L.size(); i++) {
        const sd_yolo_layer& l = y->L[i];
        if (l.type != SD_YOLO_CONV) continue;
        const int cin = i == 0 ? 3 : y->R[i].cinPad;
        n += (size_t)l.filters * (l.batch_normalize ? 4 : 1) + (size_t)l.filters * cin * l.size * l.size;
    }
    *n_floats = n;
    return SD_OK;
}

int sd_yolo_load_darknet_weights(sd_yolo* y, const float* p, size_t n_floats)
{
    if (!y || !p) return SD_ERR_INVALID;
    size_t need = 0;
    sd_yolo_weight_count(y, &need);
    if (n_floats != need) return set_err(SD_ERR_INVALID, "weight payload has " + std::to_string(n_floats) + " floats, the network needs " + std::to_string(need));
    if (y->f32) {
        // f32 mode: [coutPad][taps][cinPad] f32 (the first layer's 3 input channels sit in a K chunk of 8), batch-norm folded in f32
        std::vector<float> w32(y->wTotal, 0.f);
        std::vector<float> b32(y->bTotal, 0.f);
        const float* q = p;
        for (size_t i = 0; i < y->L.size(); i++) {
            const sd_yolo_layer& l = y->L[i];
            if (l.type != SD_YOLO_CONV) continue;
            const sd_yolo::Rt& r = y->R[i];
            const int cin = i == 0 ? 3 : r.cinPad, cinP = i == 0 ? 8 : r.cinPad, F = l.filters, taps = l.size * l.size;
            const float* biases = q; q += F;
            const float *scales = nullptr, *mean = nullptr, *var = nullptr;
            if (l.batch_normalize) { scales = q; q += F; mean = q; q += F; var = q; q += F; }
            const float* wt = q; q += (size_t)F * cin * taps;
            for (int f = 0; f < F; f++) {
                float sc = 1.f, bias = biases[f];
                if (l.batch_normalize) { sc = scales[f] / sqrtf(var[f] + 0.000001f); bias = biases[f] - mean[f] * sc; }
                b32[r.bOff + f] = bias;
                for (int c = 0; c < cin; c++)
                    for (int t = 0; t < taps; t++) {
                        // first layer: K step s = taps 2 s and 2 s + 1, four channels each (k_conv_f32's `pair` mode); else [tap][cinPad]
                        const size_t k = i == 0 ? (size_t)f * 8 * ((taps + 1) / 2) + (size_t)(t / 2) * 8 + (size_t)(t % 2) * 4 + c
                                                : ((size_t)f * taps + t) * cinP + c;
                        w32[r.wOff + k] = wt[((size_t)f * cin + c) * taps + t] * sc;
                    }
            }
        }
        HIPCHK(hipMemcpy(y->d_wgt32, w32.data(), y->wTotal * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(y->d_bias, b32.data(), y->bTotal * 4, hipMemcpyHostToDevice));
        if (y->wTotalW) {
            // SD_YOLO_F32W: U = G g G^T of the folded weights, [coutPad][16][cin]; G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
            std::vector<float> wW(y->wTotalW, 0.f);
            for (size_t i = 0; i < y->L.size(); i++) {
                const sd_yolo::Rt& r = y->R[i];
                if (r.cls != SD_YC_WINO) continue;
                const int cin = r.cinPad, F = y->L[i].filters;
                for (int f = 0; f < F; f++)
                    for (int c = 0; c < cin; c++) {
                        float g[3][3], t[4][3];
                        for (int k = 0; k < 9; k++) g[k / 3][k % 3] = w32[r.wOff + ((size_t)f * 9 + k) * cin + c];
                        for (int j = 0; j < 3; j++) {
                            t[0][j] = g[0][j];
                            t[1][j] = 0.5f * ((g[0][j] + g[1][j]) + g[2][j]);
                            t[2][j] = 0.5f * ((g[0][j] - g[1][j]) + g[2][j]);
                            t[3][j] = g[2][j];
                        }
                        for (int a = 0; a < 4; a++) {
                            const float u[4] = {t[a][0], 0.5f * ((t[a][0] + t[a][1]) + t[a][2]), 0.5f * ((t[a][0] - t[a][1]) + t[a][2]), t[a][2]};
                            for (int b = 0; b < 4; b++) wW[r.wOffW + ((size_t)f * 16 + 4 * a + b) * cin + c] = u[b];
                        }
                    }
            }
            HIPCHK(hipMemcpy(y->d_wgtW, wW.data(), y->wTotalW * 4, hipMemcpyHostToDevice));
        }
        if (y->wTotalB) {
            // SD_YOLO_F32X3: every folded weight as three bf16 limbs (round to nearest even, each limb of what the ones before left: the sum
            // of the three is the f32 weight exactly), [coutPad][taps][cin / 4][limb][4]
            auto bf16_rne = [](float v) -> uint16_t {
                uint32_t u; memcpy(&u, &v, 4);
                if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16);
                return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
            };
            auto bf16_val = [](uint16_t b) -> float { uint32_t u = (uint32_t)b << 16; float v; memcpy(&v, &u, 4); return v; };
            // fragment order: [filter tile of 128][K step][wave row (64 filters)][limb][m (32 filters)][lane = filter % 32 + 32 * (k / 8)][k % 8]
            std::vector<uint16_t> wB(y->wTotalB * 8, 0);
            for (size_t i = 0; i < y->L.size(); i++) {
                const sd_yolo::Rt& r = y->R[i];
                if (!yolo_class_b3(r.cls)) continue;
                const int cin = r.cinPad, taps = y->L[i].size * y->L[i].size, F = y->L[i].filters;
                const size_t ksteps = (size_t)taps * (cin / 16);
                const bool flat = yolo_class_b3_flat(r.cls);
                const int wm = yolo_class_b3_wm(r.cls);
                for (int f = 0; f < F; f++)
                    for (int t = 0; t < taps; t++)
                        for (int c = 0; c < cin; c++) {
                            const float v = w32[r.wOff + ((size_t)f * taps + t) * cin + c];
                            const uint16_t hi = bf16_rne(v); const float r1 = v - bf16_val(hi);
                            const uint16_t mid = bf16_rne(r1); const float r2 = r1 - bf16_val(mid);
                            const uint16_t lo = bf16_rne(r2);
                            const size_t ks = flat ? (size_t)(c / 16) * 9 + t : (size_t)t * (cin / 16) + c / 16;      // k_conv3x3_b3 walks [chunk][tap]
                            const int k = c % 16, lane = f % 32 + 32 * (k / 8), bm = 64 * wm, wmr = (f % bm) / 64, m = (f % 64) / 32;
                            const size_t frag0 = (((size_t)(f / bm) * ksteps + ks) * wm + wmr) * 6;
                            const uint16_t limb[3] = {hi, mid, lo};
                            for (int l = 0; l < 3; l++) wB[((r.wOffB + (frag0 + 2 * l + m) * 64 + lane) * 8) + k % 8] = limb[l];
                        }
            }
            HIPCHK(hipMemcpy(y->d_wgtB, wB.data(), y->wTotalB * 16, hipMemcpyHostToDevice));
        }
        y->weightsLoaded = true;
        return SD_OK;
    }
    std::vector<_Float16> w(y->wTotal, (_Float16)0.f);
    std::vector<float> b(y->bTotal, 0.f);
    for (size_t i = 0; i < y->L.size(); i++) {
        const sd_yolo_layer& l = y->L[i];
        if (l.type != SD_YOLO_CONV) continue;
        const sd_yolo::Rt& r = y->R[i];
        const int cin = i == 0 ? 3 : r.cinPad, F = l.filters, taps = l.size * l.size;
        const float* biases = p; p += F;
        const float *scales = nullptr, *mean = nullptr, *var = nullptr;
        if (l.batch_normalize) { scales = p; p += F; mean = p; p += F; var = p; p += F; }
        const float* wt = p; p += (size_t)F * cin * taps;
        for (int f = 0; f < F; f++) {
            // batch-norm folding as cv::dnn's Darknet importer applies it: y = (x - mean) * scale / sqrt(var + 1e-6) + beta
            float s = 1.f, bias = biases[f];
            if (l.batch_normalize) { s = scales[f] / sqrtf(var[f] + 0.000001f); bias = biases[f] - mean[f] * s; }
            b[r.bOff + f] = bias;
            for (int c = 0; c < cin; c++)
                for (int t = 0; t < taps; t++)
                {
                    if (i == 0)                        // k_conv_first: one 48-wide K row per filter, k = tap*4 + c
                        w[r.wOff + (size_t)f * 48 + (size_t)t * 4 + c] = (_Float16)(wt[((size_t)f * cin + c) * taps + t] * s);
                    else
                        w[r.wOff + ((size_t)f * taps + t) * r.cinPad + c] = (_Float16)(wt[((size_t)f * cin + c) * taps + t] * s);
                }
        }
    }
    HIPCHK(hipMemcpy(y->d_wgt, w.data(), y->wTotal * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(y->d_bias, b.data(), y->bTotal * 4, hipMemcpyHostToDevice));
    y->weightsLoaded = true;
    return SD_OK;
}

int sd_yolo_layer_shape(const sd_yolo* y, int layer, int* h, int* w, int* c)
{
    if (!y || layer < 0 || layer >= (int)y->L.size()) return SD_ERR_INVALID;
    if (h) *h = y->R[layer].H;
    if (w) *w = y->R[layer].W;
    if (c) *c = y->R[layer].C;
    return SD_OK;
}

int sd_yolo_flops(const sd_yolo* y, double* flops_per_image)
{
    if (!y || !flops_per_image) return SD_ERR_INVALID;
    *flops_per_image = y->convFlops;
    return SD_OK;
}

int sd_yolo_mfma_flops_bf16(const sd_yolo* y, double* flops_per_image)
{
    if (!y || !flops_per_image) return SD_ERR_INVALID;
    *flops_per_image = y->mfmaFlopsBf16;
    return SD_OK;
}

int sd_yolo_winograd_layers(const sd_yolo* y, int* n_layers)
{
    if (!y || !n_layers) return SD_ERR_INVALID;
    int n = 0;
    for (const sd_yolo::Rt& r : y->R) n += r.cls == SD_YC_WINO;
    *n_layers = n;
    return SD_OK;
}

int sd_yolo_mfma_flops(const sd_yolo* y, double* flops_per_image)
{
    if (!y || !flops_per_image) return SD_ERR_INVALID;
    *flops_per_image = y->mfmaFlops;
    return SD_OK;
}

// The forward pass: one walk over the layers for the four modes.  Which kernel runs a convolution, on which tiles and grid, is yolo_plan_launch's
// decision (sd_yolo_plan.h); here its argument struct is filled and the table row launched.
int sd_yolo_forward_device(sd_yolo* y, const uint8_t* d_bgr, int width, int height, size_t stride, size_t image_pitch, int n,
                           float conf_threshold, void* stream_)
{
    if (!y || !d_bgr || width < 2 || height < 2 || n < 1 || n > y->maxBatch || width > 8192 || height > 8192) return set_err(SD_ERR_INVALID, "bad forward arguments");
    if (!y->weightsLoaded) return set_err(SD_ERR_STATE, "detector weights not loaded");
    hipStream_t s = stream_ ? (hipStream_t)stream_ : y->stream;
    if (y->tabW != width || y->tabH != height) {
        std::vector<int16_t> ct, rt;
        yolo_resize_tables(width, height, y->netW, y->netH, ct, rt);
        HIPCHK(hipMemcpy(y->d_ct, ct.data(), ct.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(y->d_rt, rt.data(), rt.size() * 2, hipMemcpyHostToDevice));
        y->tabW = width; y->tabH = height;
    }
    const bool f32 = y->f32, ov = y->overlap;                           // overlap mode: f32-class modes only (sd_yolo_set_overlap)
    hipStream_t sb = ov ? y->sPre : s, sd = ov ? y->sPost : s;          // blobFromImage / region decodes
    if (ov && y->haveL0) HIPCHK(hipStreamWaitEvent(sb, y->evL0, 0));    // the previous pass's first convolution has read the blob
    {
        dim3 blk(64, 4), grd((y->netW + 63) / 64, (y->netH + 3) / 4, n);
        if (f32) hipLaunchKernelGGL(k_blob_from_image_f32, grd, blk, 0, sb, d_bgr, width, height, stride, image_pitch, y->d_ct, y->d_rt, y->d_blob8, y->netW, y->netH, 1);
        else hipLaunchKernelGGL(k_blob_from_image, grd, blk, 0, sb, d_bgr, width, height, stride, image_pitch, y->d_ct, y->d_rt, y->d_blob4, y->netW, y->netH, 1);
    }
    LAUNCH_CHECK(f32 ? "k_blob_from_image_f32" : "k_blob_from_image");
    if (ov) {
        HIPCHK(hipEventRecord(y->evBlob, sb));
        HIPCHK(hipStreamWaitEvent(s, y->evBlob, 0));
    }
    // the row counts are cleared ahead of the pass in the f16 mode, ahead of the first decode in the f32-class modes (overlap mode: once the
    // previous pass's NMS has read the row lists)
    bool cleared = !f32;
    if (cleared) HIPCHK(hipMemsetAsync(y->d_ndet, 0, (size_t)n * 4, s));
    int head = 0;
    bool headGuard = ov && y->haveDecoded;              // before the first head tensor is overwritten: the previous pass's decodes have read them
    const void* cur = f32 ? (const void*)y->d_blob8.get() : (const void*)y->d_blob4.get();
    int H = y->netH, W = y->netW, Cs = f32 ? 4 : 32;
    int rowBase = 0;
    for (size_t i = 0; i < y->L.size(); i++) {
        const sd_yolo_layer& l = y->L[i];
        const sd_yolo::Rt& r = y->R[i];
        if (l.type == SD_YOLO_CONV) {
            if (headGuard && i + 1 < y->L.size() && y->L[i + 1].type == SD_YOLO_YOLO) { HIPCHK(hipStreamWaitEvent(s, y->evDecoded, 0)); headGuard = false; }
            const SdYoloLaunch K = yolo_plan_launch(l, r, i == 0, n);
            const void* bias = y->d_bias + r.bOff;
            const void* res = nullptr; int resStride = 0;          // the residual of a shortcut fused into this convolution's epilogue
            if (i + 1 < y->L.size() && y->L[i + 1].type == SD_YOLO_SHORTCUT && y->R[i + 1].alias) {
                const sd_yolo::Rt& rf = y->R[yolo_resolve((int)i + 1, y->L[i + 1].from[0])];
                res = rf.out; resStride = rf.outC;
            }
            int rc;
            if (K.kernel == SD_YK_CONV_FIRST) {
                const _Float16* blob = y->d_blob4; const _Float16* wgt = y->d_wgt + r.wOff; _Float16* out = r.as<_Float16>();
                int Ho = r.H, Wo = r.W, cout = l.filters, outStride = r.outC, leaky = l.leaky;
                void* args[] = {&blob, &wgt, &bias, &out, &n, &Ho, &Wo, &cout, &outStride, &leaky};
                rc = yolo_launch(K, args, s);
            } else if (r.cls == SD_YC_F16) {
                SdConvArgs A;
                A.zero = y->d_zero; A.in = (const _Float16*)cur; A.wgt = y->d_wgt + r.wOff; A.bias = (const float*)bias; A.res = (const _Float16*)res; A.out = r.as<_Float16>();
                A.N = n; A.H = H; A.W = W; A.cin = r.cinPad; A.cinStride = Cs;
                A.Ho = r.H; A.Wo = r.W; A.cout = l.filters; A.coutPad = r.coutPad; A.outStride = r.outC; A.outOff = 0; A.resStride = resStride;
                A.ksize = l.size; A.stride = l.stride; A.pad = l.size / 2; A.leaky = l.leaky;
                void* args[] = {&A};
                rc = yolo_launch(K, args, s);
            } else if (r.cls == SD_YC_WINO) {
                // Winograd F(2x2, 3x3), k_yolo32w.h: input transform into the scratch V, then one GEMM over K = 16 cin with the output transform folded in
                SdWinoArgs A;
                A.V = y->d_V; A.U = y->d_wgtW + r.wOffW; A.bias = (const float*)bias; A.res = (const float*)res; A.out = r.as<float>(); A.zero = (const float*)y->d_zero.get();
                A.N = n; A.H = r.H; A.W = r.W; A.th = (r.H + 1) / 2; A.tw = (r.W + 1) / 2;
                A.cin = r.cinPad; A.cout = l.filters; A.outStride = r.outC; A.resStride = resStride; A.leaky = l.leaky;
                A.tilesX = K.tilesX; A.tilesY = K.tilesY; A.groupY = K.groupY;
                hipLaunchKernelGGL(k_wino_input, dim3(K.inputGrid), dim3(256), 0, s, (const float*)cur, n, H, W, r.cinPad, Cs, A.th, A.tw, y->d_V);
                LAUNCH_CHECK("k_wino_input");
                void* args[] = {&A};
                rc = yolo_launch(K, args, s);
            } else {
                SdConvArgsF A;
                A.in = (const float*)cur; A.wgt = y->d_wgt32 + r.wOff; A.bias = (const float*)bias; A.res = (const float*)res; A.out = r.as<float>(); A.zero = (const float*)y->d_zero.get();
                A.N = n; A.H = H; A.W = W; A.cin = i == 0 ? 8 : r.cinPad; A.cinStride = Cs; A.pair = i == 0 ? 1 : 0;
                A.Ho = r.H; A.Wo = r.W; A.cout = l.filters; A.outStride = r.outC; A.resStride = resStride;
                A.ksize = l.size; A.stride = l.stride; A.pad = l.size / 2; A.leaky = l.leaky;
                A.tilesX = K.tilesX; A.tilesY = K.tilesY; A.groupY = K.groupY;
                const SdF32Setup S = yolo_f32_setup(K.tilesX, K.groupY, r.H, r.W, W, l.size, Cs);
                // the kernels index pixels in 32 bits (k_conv_f32's gather: 24-bit factors) and move between taps by 32-bit byte distances
                if (S.tapRow > INT_MAX || S.tapRow < INT_MIN || (long long)n * r.H * r.W + 512 > INT_MAX || (long long)n * H * W > INT_MAX || (long long)n * H >= (1 << 23) || W >= (1 << 23))
                    return set_err(SD_ERR_UNSUPPORTED, "convolution too large for the f32 kernels' 32-bit pixel index");
                // the two unconditional tiles address their staging loads as descriptor base + 32-bit lane offset + scalar walk
                if ((K.kernel == SD_YK_F32_16_2_2_4 || K.kernel == SD_YK_F32_16_1_2_4) &&
                    !yolo_f32_walk_fits(K.kernel == SD_YK_F32_16_2_2_4 ? 128 : 256, H, W, r.H, r.W, l.size, r.cinPad, Cs))
                    return set_err(SD_ERR_UNSUPPORTED, "convolution too large for the f32 kernels' 32-bit staging offsets");
                A.mHoWo = S.hoWo.m; A.sHoWo = S.hoWo.s; A.mWo = S.wo.m; A.sWo = S.wo.s;
                A.mPerGroup = S.perGroup.m; A.sPerGroup = S.perGroup.s; A.mGroupY = S.groupY.m; A.sGroupY = S.groupY.s;
                A.tapCol = (int)S.tapCol; A.tapRow = (int)S.tapRow;
                const uint4* wq =y->d_wgtB + r.wOffB;                 // the limb kernels' second argument
                void* args[] = {&A, &wq};
                rc = yolo_launch(K, args, s);
            }
            if (rc != SD_OK) return rc;
        } else if (l.type == SD_YOLO_SHORTCUT) {
            if (!r.alias) return set_err(SD_ERR_UNSUPPORTED, "unfused [shortcut] is not implemented");      // a guard: sd_yolo_create_prec refuses such a list
        } else if (l.type == SD_YOLO_ROUTE && l.nfrom == 2) {
            const int fa = yolo_resolve((int)i, l.from[0]), fb = yolo_resolve((int)i, l.from[1]);
            const int src = yolo_resolve(fa, -1);          // the layer the [upsample] reads
            const sd_yolo::Rt& ra = y->R[src]; const sd_yolo::Rt& rb = y->R[fb];
            if (f32 && r.alias) {                          // the skip tensor was written in place by its producer: only the up-sampled half moves
                const size_t quads = (size_t)n * r.H * r.W * (ra.C / 4);
                hipLaunchKernelGGL(k_upsample_into_f32, dim3((unsigned)std::min<size_t>((quads + 255) / 256, 4096)), dim3(256), 0, s, ra.as<const float>(), ra.C, ra.outC, ra.H, ra.W,
                                   r.as<float>(), r.C, n);
                LAUNCH_CHECK("k_upsample_into_f32");
            } else {
                // the copy kernel moves 16-byte pieces of halfs: an f32 channel counts as two
                const int hc = f32 ? 2 : 1, piece = 8 / hc;
                if (ra.outC != ra.C || rb.outC != rb.C || (ra.C % piece) || (rb.C % piece))
                    return set_err(SD_ERR_UNSUPPORTED, f32 ? "route inputs must be dense, channels % 4 == 0" : "route inputs must be dense, channels % 8 == 0");
                hipLaunchKernelGGL(k_upsample_concat, dim3(2048), dim3(256), 0, s, ra.as<const _Float16>(), hc * ra.C, ra.H, ra.W, rb.as<const _Float16>(), hc * rb.C,
                                   r.as<_Float16>(), n);
                LAUNCH_CHECK("k_upsample_concat");
            }
        } else if (l.type == SD_YOLO_YOLO) {
            if (ov && head < 3) {
                HIPCHK(hipEventRecord(y->evHead[head], s));
                HIPCHK(hipStreamWaitEvent(sd, y->evHead[head], 0));
                if (head == 0 && y->haveNms) HIPCHK(hipStreamWaitEvent(sd, y->evNms, 0));     // the previous pass's NMS has read the row lists
            }
            if (!cleared) { HIPCHK(hipMemsetAsync(y->d_ndet, 0, (size_t)n * 4, sd)); cleared = true; }
            if (f32) yolo_decode<float>(y, l, r, n, conf_threshold, rowBase, sd);
            else yolo_decode<_Float16>(y, l, r, n, conf_threshold, rowBase, sd);
            LAUNCH_CHECK("k_region_decode");
            rowBase += r.H * r.W * 3;
            head++;
        }
        if (ov && i == 0) { HIPCHK(hipEventRecord(y->evL0, s)); y->haveL0 = true; }
        // the input of the next layer
        if (l.type != SD_YOLO_YOLO && l.type != SD_YOLO_UPSAMPLE) { cur = r.out; H = r.H; W = r.W; Cs = r.outC; }
        if (l.type == SD_YOLO_YOLO) { cur = r.out; }
    }
    if (!cleared) HIPCHK(hipMemsetAsync(y->d_ndet, 0, (size_t)n * 4, sd));          // a network without a [yolo] layer yields no rows
    if (ov) { HIPCHK(hipEventRecord(y->evDecoded, sd)); y->haveDecoded = true; }
    y->lastN = n;
    if (!stream_) { HIPCHK(hipStreamSynchronize(s)); if (ov) HIPCHK(hipStreamSynchronize(y->sPost)); }
    return SD_OK;
}

int sd_yolo_download_layer(sd_yolo* y, int layer, int image, uint16_t* out)
{
    if (!y || !out || layer < 0 || layer >= (int)y->L.size() || image < 0 || image >= y->lastN) return SD_ERR_INVALID;
    const sd_yolo::Rt& r = y->R[layer];
    if (!r.out) return set_err(SD_ERR_INVALID, "layer has no materialised output");
    HIPCHK(hipDeviceSynchronize());
    const size_t pix = (size_t)r.H * r.W, eb = y->f32 ? 4 : 2;       // f32 mode: `out` receives floats
    const unsigned char* src = r.as<const unsigned char>() + (size_t)image * pix * r.outC * eb;
    if (r.outC == r.C) {
        HIPCHK(hipMemcpy(out, src, pix * r.C * eb, hipMemcpyDeviceToHost));
    } else {
        HIPCHK(hipMemcpy2D(out, (size_t)r.C * eb, src, (size_t)r.outC * eb, (size_t)r.C * eb, pix, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

int sd_yolo_download_layer_stored(sd_yolo* y, int layer, int image, uint16_t* out, int* stored_channels)
{
    if (!y || !stored_channels || layer < 0 || layer >= (int)y->L.size()) return SD_ERR_INVALID;
    const sd_yolo::Rt& r = y->R[layer];
    // a tensor written in place into a route's buffer is dense (its stride is the route's): nothing of its own lies beyond its channels
    const int S = std::min(r.outC, (r.C + 31) / 32 * 32);
    *stored_channels = S;
    if (!out) return SD_OK;
    if (image < 0 || image >= y->lastN) return SD_ERR_INVALID;
    if (!r.out) return set_err(SD_ERR_INVALID, "layer has no materialised output");
    HIPCHK(hipDeviceSynchronize());
    const size_t pix = (size_t)r.H * r.W, eb = y->f32 ? 4 : 2;
    const unsigned char* src = r.as<const unsigned char>() + (size_t)image * pix * r.outC * eb;
    HIPCHK(hipMemcpy2D(out, (size_t)S * eb, src, (size_t)r.outC * eb, (size_t)S * eb, pix, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_yolo_precision(const sd_yolo* y, int* precision)
{
    if (!y || !precision) return SD_ERR_INVALID;
    *precision = y->b3 ? SD_YOLO_F32X3 : (y->wino ? SD_YOLO_F32W : (y->f32 ? SD_YOLO_F32 : SD_YOLO_F16));
    return SD_OK;
}

int sd_yolo_download_region(sd_yolo* y, float* rows, int* total_rows)
{
    if (!y || !rows || y->lastN != 1) return set_err(SD_ERR_STATE, "region rows are kept only after a forward with n == 1");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rows, y->d_raw, (size_t)y->totalRows * (5 + y->classes) * 4, hipMemcpyDeviceToHost));
    if (total_rows) *total_rows = y->totalRows;
    return SD_OK;
}

// shared by Segmentation_ / Segmentation: rows above the threshold -> int boxes -> NMSBoxes -> kept (class-filtered) indices
static int yolo_nms(sd_yolo* y, int image, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold,
                    std::vector<SdDet>& d, std::vector<YRect>& rects, std::vector<int>& kept)
{
    HIPCHK(hipDeviceSynchronize());
    int nd = 0;
    HIPCHK(hipMemcpy(&nd, y->d_ndet + image, 4, hipMemcpyDeviceToHost));
    if (nd > y->detCap) return set_err(SD_ERR_CAPACITY, "more than 8192 rows above the confidence threshold");
    d.resize(nd);
    if (nd) HIPCHK(hipMemcpy(d.data(), y->d_dets + (size_t)image * y->detCap, (size_t)nd * sizeof(SdDet), hipMemcpyDeviceToHost));
    std::sort(d.begin(), d.end(), [](const SdDet& a, const SdDet& b) { return a.row < b.row; });   // cv::dnn row order
    rects.assign(nd, YRect{0, 0, 0, 0});
    for (int i = 0; i < nd; i++) {
        if (!(d[i].conf > conf_threshold)) continue;
        const int centerX = (int)(d[i].cx * frame_cols), centerY = (int)(d[i].cy * frame_rows);
        const int width = (int)(d[i].w * frame_cols), height = (int)(d[i].h * frame_rows);
        rects[i] = YRect{centerX - width / 2, centerY - height / 2, width, height};
    }
    std::vector<int> order;
    for (int i = 0; i < nd; i++) if (d[i].conf > conf_threshold) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a].conf > d[b].conf; });
    std::vector<int> keep;
    for (int idx : order) {
        bool k = true;
        for (size_t j = 0; j < keep.size() && k; j++) k = yolo_overlap(rects[idx], rects[keep[j]]) <= nms_threshold;
        if (k) keep.push_back(idx);
    }
    kept.clear();
    for (int idx : keep) {
        const int c = d[idx].cls;     // coco.names: 0 person, 1 bicycle, 2 car, 3 motorbike ("motorcycle" never matches), 5 bus, 7 truck
        if (c == 0 || c == 1 || c == 2 || c == 5 || c == 7) kept.push_back(idx);
    }
    return SD_OK;
}

// yolov3Segment::Segmentation (yolo.cc:34-58): mask = 1 outside the dilated central halves of the kept boxes; all ones
// (and *no_target = 1) when nothing is kept.  d_mask: frame_rows x frame_cols u8 in HBM.
int sd_yolo_mask_device(sd_yolo* y, int image, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold,
                        uint8_t* d_mask, size_t stride, int* no_target, void* stream_)
{
    if (!y || !d_mask || image < 0 || image >= y->lastN || frame_cols < 1 || frame_rows < 1 || stride < (size_t)frame_cols) return SD_ERR_INVALID;
    std::vector<SdDet> d; std::vector<YRect> rects; std::vector<int> kept;
    int rc = yolo_nms(y, image, frame_cols, frame_rows, conf_threshold, nms_threshold, d, rects, kept);
    if (rc != SD_OK) return rc;
    if (kept.size() > SD_MAX_BOXES) return set_err(SD_ERR_CAPACITY, "more than SD_MAX_BOXES kept boxes");
    if (no_target) *no_target = kept.empty();
    SdMaskRects R;
    R.n = (int)kept.size();
    for (int k = 0; k < R.n; k++) {
        const YRect& b = rects[kept[k]];
        R.x0[k] = std::max(0, b.x + b.w / 4); R.x1[k] = std::min(b.x + 3 * b.w / 4, frame_cols);
        R.y0[k] = std::max(0, b.y); R.y1[k] = std::min(b.y + b.h, frame_rows);
    }
    hipStream_t s = stream_ ? (hipStream_t)stream_ : y->stream;
    hipLaunchKernelGGL(k_mask_dilate, dim3((frame_cols + 15) / 16, (frame_rows + 15) / 16), dim3(256), 0, s, R, frame_cols, frame_rows, d_mask, stride);
    LAUNCH_CHECK("k_mask_dilate");
    if (!stream_) HIPCHK(hipStreamSynchronize(s));
    return SD_OK;
}

int sd_yolo_boxes(sd_yolo* y, int image, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold, double* boxes,
                  int32_t* class_ids, float* confidences, int cap, int* n_out)
{
    if (!y || !n_out || image < 0 || image >= y->lastN || frame_cols < 1 || frame_rows < 1) return SD_ERR_INVALID;
    {
        std::vector<SdDet> d; std::vector<YRect> rects; std::vector<int> kept;
        int rc = yolo_nms(y, image, frame_cols, frame_rows, conf_threshold, nms_threshold, d, rects, kept);
        if (rc != SD_OK) return rc;
        int n = 0;
        for (int idx : kept) {
            if (n >= cap) return set_err(SD_ERR_CAPACITY, "box buffer too small");
            const YRect& r = rects[idx];
            // rectCenterScale(box, Size2d(-0.2 w, 0.6 h)): rect += size; rect -= size / 2
            const double sw = -0.2 * (double)r.w, sh = 0.6 * (double)r.h;
            if (boxes) { boxes[4 * n] = (double)r.x - sw / 2.0; boxes[4 * n + 1] = (double)r.y - sh / 2.0; boxes[4 * n + 2] = (double)r.w + sw; boxes[4 * n + 3] = (double)r.h + sh; }
            if (class_ids) class_ids[n] = d[idx].cls;
            if (confidences) confidences[n] = d[idx].conf;
            n++;
        }
        *n_out = n;
        return SD_OK;
    }
}

// Host-image forms for a per-frame caller (yolo->Segmentation_(imLeft) in the example drivers): upload + forward for one image,
// and the Segmentation mask downloaded to host memory.
int sd_yolo_forward_host(sd_yolo* y, const uint8_t* bgr, int width, int height, size_t stride, float conf_threshold)
{
    if (!y || !bgr || width < 1 || height < 1 || stride < (size_t)width * 3) return set_err(SD_ERR_INVALID, "bad yolo_forward_host arguments");
    const size_t bytes = stride * (size_t)height;
    if (bytes > y->hostImgCap) {
        y->hostImgCap = 0;
        HIPCHK(y->d_hostImg.alloc(bytes));
        y->hostImgCap = bytes;
    }
    HIPCHK(hipMemcpyAsync(y->d_hostImg, bgr, bytes, hipMemcpyHostToDevice, y->stream));
    return sd_yolo_forward_device(y, y->d_hostImg, width, height, stride, bytes, 1, conf_threshold, y->stream);
}

int sd_yolo_mask_host(sd_yolo* y, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold, uint8_t* mask, size_t stride,
                      int* no_target)
{
    if (!y || !mask || frame_cols < 1 || frame_rows < 1 || stride < (size_t)frame_cols) return set_err(SD_ERR_INVALID, "bad yolo_mask_host arguments");
    const size_t bytes = (size_t)frame_cols * frame_rows;
    if (bytes > y->hostMaskCap) {
        y->hostMaskCap = 0;
        HIPCHK(y->d_hostMask.alloc(bytes));
        y->hostMaskCap = bytes;
    }
    int rc = sd_yolo_mask_device(y, 0, frame_cols, frame_rows, conf_threshold, nms_threshold, y->d_hostMask, (size_t)frame_cols, no_target, nullptr);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemcpy2D(mask, stride, y->d_hostMask, (size_t)frame_cols, (size_t)frame_cols, (size_t)frame_rows, hipMemcpyDeviceToHost));
    return SD_OK;
}

// postprocess_ for the first n_images of the last forward pass, entirely on the device (k_yolo_nms): one launch, and
// with the host form one download of n_images x (SD_MAX_BOXES boxes + count) instead of a synchronisation per image.
int sd_yolo_boxes_device(sd_yolo* y, int n_images, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold,
                         double* d_boxes, int32_t* d_class_ids, float* d_confidences, int32_t* d_n_boxes, void* stream_)
{
    if (!y || n_images < 0 || n_images > y->lastN || frame_cols < 1 || frame_rows < 1 || !d_boxes || !d_class_ids || !d_confidences || !d_n_boxes)
        return set_err(SD_ERR_INVALID, "bad yolo_boxes_device arguments");
    if (n_images == 0) return SD_OK;
    hipStream_t s = stream_ ? (hipStream_t)stream_ : y->stream;
    if (y->overlap && y->haveDecoded) HIPCHK(hipStreamWaitEvent(s, y->evDecoded, 0));      // the decodes of the last pass (internal stream)
    hipLaunchKernelGGL(k_yolo_nms, dim3(n_images), dim3(256), SD_NMS_LDS, s, y->d_dets, y->d_ndet, y->detCap, frame_cols, frame_rows, conf_threshold,
                       nms_threshold, d_boxes, d_class_ids, d_confidences, d_n_boxes);
    LAUNCH_CHECK("k_yolo_nms");
    if (y->overlap) { HIPCHK(hipEventRecord(y->evNms, s)); y->haveNms = true; }
    return SD_OK;
}

int sd_yolo_boxes_batch(sd_yolo* y, int n_images, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold,
                        double* boxes, int32_t* class_ids, float* confidences, int32_t* n_boxes, void* stream_)
{
    if (!y || !boxes || !n_boxes || n_images < 0 || n_images > y->maxBatch) return set_err(SD_ERR_INVALID, "bad yolo_boxes_batch arguments");
    if (!y->d_nmsBoxes) {
        const size_t nB = (size_t)y->maxBatch;
        SdDevBuf<double> boxesBuf; SdDevBuf<int> cls, nBuf; SdDevBuf<float> conf;
        HIPCHK(boxesBuf.alloc(nB * SD_MAX_BOXES * 4 * 8)); HIPCHK(cls.alloc(nB * SD_MAX_BOXES * 4));
        HIPCHK(conf.alloc(nB * SD_MAX_BOXES * 4)); HIPCHK(nBuf.alloc(nB * 4));
        y->d_nmsCls = std::move(cls); y->d_nmsConf = std::move(conf); y->d_nmsN = std::move(nBuf); y->d_nmsBoxes = std::move(boxesBuf);    // boxes last: they mark the group
    }
    int rc = sd_yolo_boxes_device(y, n_images, frame_cols, frame_rows, conf_threshold, nms_threshold, y->d_nmsBoxes, y->d_nmsCls, y->d_nmsConf,
                                  y->d_nmsN, stream_);
    if (rc != SD_OK || n_images == 0) return rc;
    hipStream_t s = stream_ ? (hipStream_t)stream_ : y->stream;
    HIPCHK(hipMemcpyAsync(boxes, y->d_nmsBoxes, (size_t)n_images * SD_MAX_BOXES * 4 * 8, hipMemcpyDeviceToHost, s));
    if (class_ids) HIPCHK(hipMemcpyAsync(class_ids, y->d_nmsCls, (size_t)n_images * SD_MAX_BOXES * 4, hipMemcpyDeviceToHost, s));
    if (confidences) HIPCHK(hipMemcpyAsync(confidences, y->d_nmsConf, (size_t)n_images * SD_MAX_BOXES * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_boxes, y->d_nmsN, (size_t)n_images * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < n_images; i++)
        if (n_boxes[i] < 0) return set_err(SD_ERR_CAPACITY, "postprocess on device: more than 4096 rows above the threshold or more than SD_MAX_BOXES kept boxes");
    return SD_OK;
}


}  // extern "C"
