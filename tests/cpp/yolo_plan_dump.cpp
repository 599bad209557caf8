// Prints what csrc/sd_yolo_plan.h plans for a layer list: one line per convolution of every case "precision net_w net_h n" given on the
// command line.  The header is pure host code: this file is compiled with g++ alone.
//   yolo_plan_dump CASE...                    the built-in YOLOv3 layer list (tests/test_yolo_plan.py)
//   yolo_plan_dump --layers FILE CASE...      the layer list of FILE (tests/yolo_cases.py; "--layers FILE CASE..." may repeat): one layer per line, twelve integers
//                                             "type filters size stride batch_normalize leaky from0 from1 nfrom mask0 mask1 mask2"; after a case's
//                                             convolutions one line "route|layer|inplace" or "route|layer|copy" per 2-input [route], and a list
//                                             that creation refuses prints "refused|code|text" in place of its records
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sd_yolo_plan.h"

int main(int argc, char** argv)
{
    std::vector<sd_yolo_layer> L;
    int a = 1;
    bool file = false;
    auto load = [&](const char* path) {
        FILE* f = fopen(path, "r");
        if (!f) return false;
        L.clear();
        int v[12];
        while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11) == 12) {
            sd_yolo_layer l = {};
            l.type = v[0]; l.filters = v[1]; l.size = v[2]; l.stride = v[3]; l.batch_normalize = v[4]; l.leaky = v[5];
            l.from[0] = v[6]; l.from[1] = v[7]; l.nfrom = v[8]; l.mask[0] = v[9]; l.mask[1] = v[10]; l.mask[2] = v[11];
            L.push_back(l);
        }
        fclose(f);
        return true;
    };
    if (!(argc > 1 && !strcmp(argv[1], "--layers"))) yolo_v3_layers(L);
    for (; a + 1 < argc; a += 4) {
        if (!strcmp(argv[a], "--layers")) {               // the cases that follow are planned for this file's list ("--layers FILE" may be given again)
            if (!load(argv[a + 1])) { fprintf(stderr, "cannot read %s\n", argv[a + 1]); return 1; }
            file = true; a -= 2;
            continue;
        }
        if (a + 3 >= argc) break;
        const int prec = atoi(argv[a]), W = atoi(argv[a + 1]), H = atoi(argv[a + 2]), n = atoi(argv[a + 3]);
        SdYoloNetPlan P;
        SdYoloStorage S;
        SdYoloPlanError e = yolo_plan_net(L.data(), (int)L.size(), W, H, 80, prec, P);
        if (e.code == SD_OK) e = yolo_plan_storage(L.data(), (int)L.size(), P, prec != SD_YOLO_F16, S);
        printf("case %d %d %d %d\n", prec, W, H, n);
        if (e.code != SD_OK) {
            if (file) { printf("refused|%d|%s\n", e.code, e.text); continue; }
            fprintf(stderr, "plan error %d: %s\n", e.code, e.text); return 1;
        }
        for (size_t i = 0; i < L.size(); i++) {
            if (L[i].type != SD_YOLO_CONV) continue;
            const SdYoloLaunch K = yolo_plan_launch(L[i], P.R[i], i == 0, n);
            // layer | kernel | gridX gridY block tilesX tilesY groupY width inputGrid | filters size cinPad class
            printf("%zu|%s|%u %u %d %d %d %d %d %u|%d %d %d %d\n", i, kYoloKernelInfo[K.kernel].name, K.gridX, K.gridY, K.block, K.tilesX, K.tilesY, K.groupY,
                   K.width, K.inputGrid, L[i].filters, L[i].size, P.R[i].cinPad, P.R[i].cls);
        }
        for (size_t i = 0; file && i < L.size(); i++)
            if (L[i].type == SD_YOLO_ROUTE && L[i].nfrom == 2) printf("route|%zu|%s\n", i, S.inPlace[i] ? "inplace" : "copy");
    }
    return 0;
}
