// Prints what csrc/sd_yolo_plan.h plans for the built-in YOLOv3 layer list (tests/test_yolo_plan.py): one line per convolution of every
// case "precision net_w net_h n" given on the command line.  The header is pure host code: this file is compiled with g++ alone.
#include <cstdio>
#include <cstdlib>
#include "sd_yolo_plan.h"

int main(int argc, char** argv)
{
    std::vector<sd_yolo_layer> L;
    yolo_v3_layers(L);
    for (int a = 1; a + 3 < argc; a += 4) {
        const int prec = atoi(argv[a]), W = atoi(argv[a + 1]), H = atoi(argv[a + 2]), n = atoi(argv[a + 3]);
        SdYoloNetPlan P;
        const SdYoloPlanError e = yolo_plan_net(L.data(), (int)L.size(), W, H, 80, prec, P);
        if (e.code != SD_OK) { fprintf(stderr, "plan error %d: %s\n", e.code, e.text); return 1; }
        printf("case %d %d %d %d\n", prec, W, H, n);
        for (size_t i = 0; i < L.size(); i++) {
            if (L[i].type != SD_YOLO_CONV) continue;
            const SdYoloLaunch K = yolo_plan_launch(L[i], P.R[i], i == 0, n);
            // layer | kernel | gridX gridY block tilesX tilesY groupY width inputGrid | filters size cinPad class
            printf("%zu|%s|%u %u %d %d %d %d %d %u|%d %d %d %d\n", i, kYoloKernelInfo[K.kernel].name, K.gridX, K.gridY, K.block, K.tilesX, K.tilesY, K.groupY,
                   K.width, K.inputGrid, L[i].filters, L[i].size, P.R[i].cinPad, P.R[i].cls);
        }
    }
    return 0;
}
