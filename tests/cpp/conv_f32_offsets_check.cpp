// The staging addresses of k_conv_f32's two unconditional tiles (<16, 2, 2, 4>: 128 filters x 128 pixels, <16, 1, 2, 4>: 64 filters x 256 pixels;
// csrc/k_yolo32.h, "The scalar walk"), walked on the host: descriptor base + per-lane 32-bit offset + scalar offset against the 64-bit address of
// the gather's plain formula, for every tile, chunk, tap and K step of every layer these tiles run.  Pure host code (g++ alone);
// tests/test_conv_f32_offsets.py runs it.
//   conv_f32_offsets_check CASE...                    the built-in YOLOv3 layer list, CASE = "net_w net_h n"
//   conv_f32_offsets_check --layers FILE CASE...      the layer list of FILE (as tests/cpp/yolo_plan_dump.cpp reads it; may repeat)
// Per layer, ONCE (the walk is the same in every workgroup): the request sequence as the kernel issues it -- 1 + NSET requests in the prologue,
// one per K step -- with the scalar offsets, the tap bit and the record counts it has at each request:
//   request r < ksteps    live descriptors; the weights' scalar offset is 4 (tap cin + c0), the activations' is the byte distance from tap (0, 0),
//                         channel 0 to (tap, c0) and is never negative; the tap bit is bit `tap`;
//   request r >= ksteps   both record counts are zero (nothing is read whatever the offsets are).
// Per tile, thread, chunk, tap and step:
//   live lane (the tap lies inside the image and the pixel exists)    anchor + lane offset + scalar offset == the plain 64-bit address;
//                         lane offset in [0, 2^31); lane offset + scalar offset + 16 <= the record count (in range whether or not the
//                         hardware adds the scalar offset before its range check);
//   masked lane           the selected offset is SD_F32_WALK_SENTINEL, at or beyond the record count;
//   weights               base + lane offset + scalar offset == the filter row's address, + 16 <= the tile's BM rows.
// The anchor is formed in 64 bits from a 32-bit pixel index, as the kernel forms it: batch 256 at 640 x 480 puts the first layers' tensors beyond
// 4 GiB.  Exit status 0 and one line per case, or the first mismatch and status 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "sd_yolo_plan.h"

namespace {
constexpr int BK = 16, NT = 256, CPR = BK / 4;

struct Layer {
    int idx, BN, BM, NSET, N, H, W, cin, cs, Ho, Wo, ksize, stride, pad, tilesX, tilesY;
    long long tapCol, tapRow;
};
struct Request { int wsoff, xsoff, wrec; unsigned xrec; unsigned tapbit; };

std::atomic<bool> failed{false};
void fail(const Layer& L, const char* what, long long a, long long b, long long c, long long d)
{
    if (!failed.exchange(true)) fprintf(stderr, "layer %d (n %d, %d x %d -> %d x %d, cin %d): %s: %lld %lld %lld %lld\n", L.idx, L.N, L.W, L.H, L.Wo, L.Ho, L.cin, what, a, b, c, d);
}

// the kernel's request()/advance()/retap() on its scalar state, for the 1 + NSET + ksteps requests of a tile
std::vector<Request> requests(const Layer& L)
{
    const int taps = L.ksize * L.ksize, ksteps = taps * (L.cin / BK), wrow = taps * L.cin;
    std::vector<Request> R;
    int wsoff = 0, xsoff = 0, nreq = 0, c0 = 0, kw = 0, wrec = L.BM * wrow * 4;
    unsigned xrec = SD_F32_WALK_RECORDS, tapbit = 1;
    for (int r = 0; r < ksteps + 1 + L.NSET; r++) {
        R.push_back({wsoff, xsoff, wrec, xrec, tapbit});
        wsoff += 4 * BK; xsoff += 4 * BK;                                // request()
        nreq++; c0 += BK;                                                // advance()
        if (c0 == L.cin) {
            c0 = 0;
            kw++;                                                        // retap()
            const bool wrap = kw == L.ksize;
            if (wrap) kw = 0;
            xsoff += (int)(wrap ? L.tapRow : L.tapCol) - 4 * L.cin;
            tapbit <<= 1;
            if (nreq >= ksteps) { wrec = 0; xrec = 0; }
        }
    }
    return R;
}

bool check_requests(const Layer& L, const std::vector<Request>& R)
{
    const int taps = L.ksize * L.ksize, spt = L.cin / BK, ksteps = taps * spt, wrow = taps * L.cin;
    for (int r = 0; r < (int)R.size(); r++) {
        if (r >= ksteps) {
            if (R[r].wrec != 0 || R[r].xrec != 0) { fail(L, "a request behind the last stage has records", r, R[r].wrec, R[r].xrec, 0); return false; }
            continue;
        }
        const int t = r / spt, c0 = (r % spt) * BK, ky = t / L.ksize, kx = t % L.ksize;
        const long long xd = (((long long)ky * L.W + kx) * L.cs + c0) * 4;
        if (R[r].wrec != L.BM * wrow * 4 || R[r].xrec != SD_F32_WALK_RECORDS) { fail(L, "a live request has no records", r, R[r].wrec, R[r].xrec, 0); return false; }
        if (R[r].tapbit != 1u << t) { fail(L, "tap bit", r, R[r].tapbit, t, 0); return false; }
        if (R[r].wsoff != (t * L.cin + c0) * 4) { fail(L, "weights' scalar offset", r, R[r].wsoff, (t * L.cin + c0) * 4, 0); return false; }
        if (R[r].xsoff != xd || R[r].xsoff < 0) { fail(L, "activations' scalar offset", r, R[r].xsoff, xd, 0); return false; }
    }
    return true;
}

struct Counts { long long live = 0, masked = 0, weights = 0; };

void walk_tile(const Layer& L, const std::vector<int>& XS, int tx, Counts& C)
{
    const int taps = L.ksize * L.ksize, spt = L.cin / BK, HoWo = L.Ho * L.Wo, XC = L.BN * CPR / NT;
    const int pix0 = tx * L.BN;
    // the anchor, as the kernel forms it: a 32-bit pixel index, the byte offset in 64 bits
    const unsigned n0 = (unsigned)pix0 / HoWo, pr0 = pix0 - n0 * HoWo, y0 = pr0 / L.Wo, x0 = pr0 - y0 * L.Wo;
    const int pixelA = ((int)(n0 * L.H) + ((int)y0 * L.stride - L.pad)) * L.W + ((int)x0 * L.stride - L.pad);
    const long long anchor = (long long)pixelA * (4 * L.cs);
    // the threads of one pixel row (tid / CPR) share their pixels: the split runs once per (row, chunk), the walk once per thread
    for (int row = 0; row < NT / CPR; row++)
        for (int i = 0; i < XC; i++) {
            const unsigned p = (unsigned)pix0 + row + (NT / CPR) * i;                                    // < 2^31: the host refuses larger batches
            const unsigned n = p / (unsigned)HoWo, prr = p - n * HoWo, yo = prr / (unsigned)L.Wo, xo = prr - yo * L.Wo;
            const int yi = (int)yo * L.stride - L.pad, xi = (int)xo * L.stride - L.pad;
            const int pixel = (int)(n * (unsigned)L.H + yi) * L.W + xi;                                  // the kernel's 32-bit index (wraps only where n >= N)
            for (int q = 0; q < CPR; q++) {
                const int tid = row * CPR + q;
                const unsigned xoff = (unsigned)(pixel - pixelA) * (unsigned)(4 * L.cs) + 16u * q;
                for (int t = 0; t < taps; t++) {
                    const int ky = t / L.ksize, kx = t % L.ksize;
                    const bool live = n < (unsigned)L.N && yi + ky >= 0 && yi + ky < L.H && xi + kx >= 0 && xi + kx < L.W;
                    const unsigned voff = live ? xoff : SD_F32_WALK_SENTINEL;                               // select()
                    if (!live) {
                        if (voff < SD_F32_WALK_RECORDS) { fail(L, "a masked tap's offset lies inside the records", tx, tid, i, t); return; }
                        C.masked += spt;
                        continue;
                    }
                    if (xoff >= 0x80000000u) { fail(L, "a live lane's offset is outside [0, 2^31)", tx, tid, i, xoff); return; }
                    // the plain formula: pixel (n, yi + ky, xi + kx), channel c0 + 4 q of a tensor of cs stored channels, in bytes from its start
                    const long long want0 = ((((long long)n * L.H + yi + ky) * L.W + xi + kx) * L.cs) * 4 + 16 * q;
                    // every step of the tap (the live requests' record count is SD_F32_WALK_RECORDS: check_requests): the comparisons of all steps
                    // are folded into one flag, and the first failing step is looked up only when it is set
                    const int* xs = XS.data() + t * spt;
                    const long long got0 = anchor + (long long)voff;
                    long long diff = 0;
                    int far = 0;
                    for (int s = 0; s < spt; s++) { diff |= (got0 + xs[s]) ^ (want0 + 4ll * BK * s); far = std::max(far, xs[s]); }
                    if (diff != 0 || (long long)voff + far + 16 > (long long)SD_F32_WALK_RECORDS) {
                        for (int s = 0; s < spt; s++) {
                            if (got0 + xs[s] != want0 + 4ll * BK * s) { fail(L, "address", tx, tid, got0 + xs[s], want0 + 4ll * BK * s); return; }
                            if ((long long)voff + xs[s] + 16 > (long long)SD_F32_WALK_RECORDS) { fail(L, "a live lane leaves the records", tx, tid, voff, xs[s]); return; }
                        }
                    }
                    C.live += spt;
                }
            }
        }
}

void walk_weights(const Layer& L, const std::vector<Request>& R, Counts& C)
{
    const int taps = L.ksize * L.ksize, spt = L.cin / BK, ksteps = taps * spt, wrow = taps * L.cin, WC = L.BM * CPR / NT;
    for (int ty = 0; ty < L.tilesY; ty++) {
        const long long base = (long long)ty * L.BM * wrow * 4;
        for (int tid = 0; tid < NT; tid++)
            for (int i = 0; i < WC; i++) {
                const int row = tid / CPR + (NT / CPR) * i, q = tid % CPR;
                const unsigned woff = (unsigned)(row * wrow) * 4u + 16u * q;
                for (int r = 0; r < ksteps; r++) {
                    const int t = r / spt, c0 = (r % spt) * BK;
                    const long long got = base + woff + R[r].wsoff, want = (((long long)ty * L.BM + row) * wrow + (long long)t * L.cin + c0) * 4 + 16 * q;
                    if (got != want || (long long)woff + R[r].wsoff + 16 > R[r].wrec) { fail(L, "weights' address", ty, tid, got, want); return; }
                }
                C.weights += ksteps;
            }
    }
}

bool walk_layer(const Layer& L, Counts& C)
{
    if (!yolo_f32_walk_fits(L.BN, L.H, L.W, L.Ho, L.Wo, L.ksize, L.cin, L.cs)) { fail(L, "yolo_f32_walk_fits refuses the layer", 0, 0, 0, 0); return false; }
    const std::vector<Request> R = requests(L);
    if (!check_requests(L, R)) return false;
    walk_weights(L, R, C);
    unsigned nth = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    if (L.tilesX < 64) nth = 1;
    std::vector<Counts> part(nth);
    std::vector<std::thread> T;
    std::atomic<int> next{0};
    std::vector<int> XS;                                 // the activations' scalar offset at every live request
    for (int r = 0; r < L.ksize * L.ksize * (L.cin / BK); r++) XS.push_back(R[r].xsoff);
    auto work = [&](int k) { for (int tx; !failed && (tx = next++) < L.tilesX;) walk_tile(L, XS, tx, part[k]); };
    for (unsigned k = 1; k < nth; k++) T.emplace_back(work, (int)k);
    work(0);
    for (auto& t : T) t.join();
    for (const Counts& c : part) { C.live += c.live; C.masked += c.masked; }
    return !failed;
}
}

int main(int argc, char** argv)
{
    std::vector<sd_yolo_layer> L;
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
    int a = 1;
    if (!(argc > 1 && !strcmp(argv[1], "--layers"))) yolo_v3_layers(L);
    while (a < argc) {
        if (!strcmp(argv[a], "--layers")) {
            if (a + 1 >= argc || !load(argv[a + 1])) { fprintf(stderr, "cannot read the layer list\n"); return 1; }
            a += 2;
            continue;
        }
        if (a + 2 >= argc) { fprintf(stderr, "a case is \"net_w net_h n\"\n"); return 1; }
        const int netW = atoi(argv[a]), netH = atoi(argv[a + 1]), n = atoi(argv[a + 2]);
        a += 3;
        SdYoloNetPlan P;
        const SdYoloPlanError e = yolo_plan_net(L.data(), (int)L.size(), netW, netH, 80, SD_YOLO_F32, P);
        if (e.code != SD_OK) { fprintf(stderr, "plan error %d: %s\n", e.code, e.text); return 1; }
        // the layer walk of sd_yolo_forward: the map and the stored channel count a convolution reads
        int H = netH, W = netW, Cs = 4, layers = 0;
        long long tiles = 0;
        Counts C;
        for (size_t i = 0; i < L.size(); i++) {
            const sd_yolo_layer& l = L[i];
            const SdYoloLayerPlan& r = P.R[i];
            if (l.type == SD_YOLO_CONV) {
                const SdYoloLaunch K = yolo_plan_launch(l, r, i == 0, n);
                if (K.kernel == SD_YK_F32_16_2_2_4 || K.kernel == SD_YK_F32_16_1_2_4) {
                    const bool big = K.kernel == SD_YK_F32_16_2_2_4;
                    const SdF32Setup S = yolo_f32_setup(K.tilesX, K.groupY, r.H, r.W, W, l.size, Cs);
                    const Layer Y = {(int)i, big ? 128 : 256, big ? 128 : 64, big ? 2 : 1, n, H, W, r.cinPad, Cs, r.H, r.W, l.size, l.stride, l.size / 2, K.tilesX, K.tilesY, S.tapCol, S.tapRow};
                    if (!walk_layer(Y, C)) return 1;
                    layers++; tiles += (long long)K.tilesX * K.tilesY;
                }
            }
            if (l.type != SD_YOLO_YOLO && l.type != SD_YOLO_UPSAMPLE) { H = r.H; W = r.W; Cs = r.outC; }
        }
        printf("%d x %d n=%d: %d layers, %lld tiles, %lld live and %lld masked activation requests, %lld weight requests: ok\n", netW, netH, n, layers, tiles, C.live, C.masked, C.weights);
    }
    return 0;
}
