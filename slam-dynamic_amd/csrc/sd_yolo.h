// Host side of the detector behind the C ABI (included by sd_yolo_api.hip): the detector object, the resize tables and the
// reference's post-processing helpers.  The network description and the choice of kernels: sd_yolo_plan.h.
//   yolov3Segment::yolov3Segment / readNetFromDarknet     src/yolo.cc:15-31
//   yolov3Segment::Segmentation_                          src/yolo.cc:60-77
//   yolov3Segment::postprocess_ + rectCenterScale         src/yolo.cc:142-206
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "k_yolo.h"
#include "k_yolo32.h"
#include "k_yolo32w.h"
#include "k_yolo32b.h"
#include "sd_common.h"
#include "sd_yolo_plan.h"

struct sd_yolo : SdYoloTotals {          // sizes and FLOP totals: yolo_plan_net (sd_yolo_plan.h)
    std::vector<sd_yolo_layer> L;
    struct Rt : SdYoloLayerPlan {        // a layer's shape record plus where its output lives; outC becomes the route's channel count when a 2-input [route] owns the storage
        Rt(const SdYoloLayerPlan& p) : SdYoloLayerPlan(p) {}
        void* out = nullptr;             // activations, _Float16 in the f16 mode and float in the f32-class modes: read through as<T>()
        bool alias = false;
        SdDevBuf<unsigned char> own;     // output storage allocated for this layer; `out` may point into another layer's (alias)
        template <typename T> T* as() const { return (T*)out; }
    };
    std::vector<Rt> R;
    int netW = 0, netH = 0, classes = 80, maxBatch = 0;
    int f32 = 0;                   // SD_YOLO_F32: activations / weights / arithmetic in f32 (k_yolo32.h)
    SdDevBuf<float> d_blob8; SdDevBuf<float> d_wgt32;
    int wino = 0;                  // SD_YOLO_F32W (k_yolo32w.h): f32 mode with the eligible 3 x 3 stride-1 layers as Winograd F(2x2, 3x3)
    SdDevBuf<float> d_wgtW; SdDevBuf<float> d_V;
    int b3 = 0;                    // SD_YOLO_F32X3 (k_yolo32b.h): f32 mode with the >= 64-filter layers on three bf16 limbs per operand
    SdDevBuf<uint4> d_wgtB;
    float anchors[18];
    SdDevBuf<_Float16> d_blob4;   // network input, NHWC f16 x 4 channels
    SdDevBuf<_Float16> d_wgt; SdDevBuf<float> d_bias; SdDevBuf<_Float16> d_zero;
    SdDevBuf<short4> d_ct; SdDevBuf<short4> d_rt;
    SdDevBuf<SdDet> d_dets; SdDevBuf<int> d_ndet; SdDevBuf<float> d_raw;
    SdDevBuf<uint8_t> d_hostImg; size_t hostImgCap = 0; SdDevBuf<uint8_t> d_hostMask; size_t hostMaskCap = 0;      // sd_yolo_forward_host / mask_host
    SdDevBuf<double> d_nmsBoxes; SdDevBuf<int> d_nmsCls; SdDevBuf<float> d_nmsConf; SdDevBuf<int> d_nmsN;      // sd_yolo_boxes_batch
    int detCap = 0;
    int tabW = 0, tabH = 0;
    bool weightsLoaded = false;
    int lastN = 0;
    hipStream_t stream = nullptr;
    // overlap mode (sd_yolo_set_overlap, f32-class modes): blobFromImage of a pass on sPre, the region decodes on sPost, ordered against the convolution
    // stream by events, so that with two passes enqueued the next pass's convolutions start while this pass's decode / NMS / download still run
    bool overlap = false, haveL0 = false, haveDecoded = false, haveNms = false;
    hipStream_t sPre = nullptr, sPost = nullptr;
    hipEvent_t evBlob = nullptr, evL0 = nullptr, evHead[3] = {nullptr, nullptr, nullptr}, evDecoded = nullptr, evNms = nullptr;
    ~sd_yolo()
    {
        for (hipStream_t q : {stream, sPre, sPost}) if (q) (void)hipStreamDestroy(q);
        for (hipEvent_t e : {evBlob, evL0, evHead[0], evHead[1], evHead[2], evDecoded, evNms}) if (e) (void)hipEventDestroy(e);
    }
};

// cv::resize INTER_LINEAR coefficient tables (same fixed-point scheme as the pyramid, sd_plan.h)
static void yolo_resize_tables(int sw, int sh, int dw, int dh, std::vector<int16_t>& ct, std::vector<int16_t>& rt)
{
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    ct.assign(4 * (size_t)dw, 0); rt.assign(4 * (size_t)dh, 0);
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        ct[4 * dx] = (int16_t)sx; ct[4 * dx + 1] = (int16_t)lrintf((1.f - fx) * 2048); ct[4 * dx + 2] = (int16_t)lrintf(fx * 2048);
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floorf(fy);
        fy -= sy;
        rt[4 * dy] = (int16_t)sy; rt[4 * dy + 1] = (int16_t)lrintf((1.f - fy) * 2048); rt[4 * dy + 2] = (int16_t)lrintf(fy * 2048);
    }
}

struct YRect { int x, y, w, h; };
static inline float yolo_overlap(const YRect& a, const YRect& b)
{
    // 1 - jaccardDistance(a, b) of cv::Rect (integer areas, double ratio)
    const double Aa = (double)a.w * a.h, Ab = (double)b.w * b.h;
    if ((Aa + Ab) <= 2.220446049250313e-16) return 1.f;
    const int x1 = std::max(a.x, b.x), y1 = std::max(a.y, b.y);
    const int x2 = std::min(a.x + a.w, b.x + b.w), y2 = std::min(a.y + a.h, b.y + b.h);
    const double Aab = (x2 > x1 && y2 > y1) ? (double)(x2 - x1) * (y2 - y1) : 0.0;
    return (float)(1. - (1. - Aab / (Aa + Ab - Aab)));
}
