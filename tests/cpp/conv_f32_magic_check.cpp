// Walks, for every convolution of the built-in YOLOv3 list in every case "net_w net_h n" of the command line, the four divisions k_conv_f32's
// set-up does by multiply-high (yolo_f32_setup, csrc/sd_yolo_plan.h) over their FULL ranges -- pixels [0, npix + tile) by Ho Wo and the remainders
// [0, Ho Wo) by Wo, workgroup slots [0, grid / 8) by perXcd groupY and the remainders by groupY -- against plain division
// (tests/test_conv_f32_magic_div.py).  Prints one line per case: "case W H n: <divisions checked> checked, <mismatches> wrong".  Pure host code.
#include <cstdio>
#include <cstdlib>
#include "sd_yolo_plan.h"

static unsigned long long walk(unsigned d, SdMagic k, unsigned long long range, unsigned long long& bad)
{
    for (unsigned long long n = 0; n < range; n++) bad += sd_magic_quot((unsigned)n, k) != (unsigned)n / d;
    return range;
}

int main(int argc, char** argv)
{
    std::vector<sd_yolo_layer> L;
    yolo_v3_layers(L);
    int rc = 0;
    {   // the ends of the range the formula is stated for: divisors 1, 2, 3, powers of two and their neighbours up to 2^31 - 1, dividends at the
        // multiples of d nearest to 0, 2^30 and 2^31 - 1 (the quotient's error, if any, first shows one below a multiple)
        unsigned long long checked = 0, bad = 0;
        std::vector<unsigned> ds = {1, 2, 3, 5, 7, 9, 307200, 76800, 640, 0x7fffffffu};
        for (int b = 2; b < 31; b++) { ds.push_back((1u << b) - 1); ds.push_back(1u << b); ds.push_back((1u << b) + 1); }
        for (unsigned d : ds)
            for (unsigned long long c : {0ull, 1ull << 30, 0x7fffffffull}) {
                const unsigned long long m = c / d * d;
                for (long long n = (long long)m - 2; n <= (long long)(m + d) + 2; n += (n == (long long)m + 2 && d > 8 ? d - 4 : 1)) {
                    if (n < 0 || n > 0x7fffffffll) continue;
                    checked++; bad += sd_magic_quot((unsigned)n, sd_magic_div(d)) != (unsigned)n / d;
                }
            }
        printf("edges: %llu checked, %llu wrong\n", checked, bad);
        if (bad) rc = 2;
    }
    for (int a = 1; a + 2 < argc; a += 3) {
        const int W = atoi(argv[a]), H = atoi(argv[a + 1]), n = atoi(argv[a + 2]);
        SdYoloNetPlan P;
        const SdYoloPlanError e = yolo_plan_net(L.data(), (int)L.size(), W, H, 80, SD_YOLO_F32, P);
        if (e.code != SD_OK) { fprintf(stderr, "plan error %d: %s\n", e.code, e.text); return 1; }
        unsigned long long checked = 0, bad = 0;
        int inW = W;
        for (size_t i = 0; i < L.size(); i++) {
            if (L[i].type == SD_YOLO_CONV) {
                const SdYoloLaunch K = yolo_plan_launch(L[i], P.R[i], i == 0, n);
                const int Ho = P.R[i].H, Wo = P.R[i].W;
                const SdF32Setup S = yolo_f32_setup(K.tilesX, K.groupY, Ho, Wo, inW, L[i].size, 4);
                const unsigned perGroup = (unsigned)(((K.tilesX + 7) / 8) * K.groupY);
                checked += walk((unsigned)(Ho * Wo), S.hoWo, (unsigned long long)n * Ho * Wo + 512, bad);     // + the widest pixel tile: the last tile's rows beyond npix
                checked += walk((unsigned)Wo, S.wo, (unsigned long long)Ho * Wo, bad);
                checked += walk(perGroup, S.perGroup, K.gridX / 8, bad);
                checked += walk((unsigned)K.groupY, S.groupY, perGroup, bad);
            }
            if (L[i].type != SD_YOLO_YOLO) inW = P.R[i].W;
        }
        printf("case %d %d %d: %llu checked, %llu wrong\n", W, H, n, checked, bad);
        if (bad) rc = 2;
    }
    return rc;
}
