// The detector in the reference's own arithmetic: f32 operands, f32 accumulation, on v_mfma_f32_32x32x2_f32 (dense peak
// 157.3 TFLOP/s, 1/16 of the f16 rate).  cv::dnn runs YOLOv3 in f32 on the CPU (src/yolo.cc:29 DNN_TARGET_CPU); this mode
// exists so that the box sets can be compared with an f32 forward pass instead of being explained away by a tolerance, and
// so that the f16 mode's disagreements can be counted against it (tests/test_gpu_yolo.py).  Activations NHWC f32, weights
// [coutPad][taps][cin] f32 with batch-norm folded in f32.
//   k_blob_from_image_f32   blobFromImage -> NHWC f32 x 4 channels (R, G, B, 0: one 16-byte piece per pixel; the first layer pairs two
//                           filter taps into one 8-wide K chunk, see `pair` below)
//   k_conv_f32<BK, WM, MT, NW>   implicit-GEMM convolution, 1x1 / 3x3, stride 1 / 2, + bias + leaky ReLU + shortcut
//   k_upsample_into_f32     the up-sampled half of a 2-input [route] whose other half its producer wrote in place
// One f32 MFMA is 64 cycles for 4096 FLOPs and needs ONE float per operand per lane, so the kernel is MFMA-bound with a
// plain structure: NW waves, K walked in steps of BK channels of one filter tap, tiles staged through registers into LDS.  A lane reads
// its fragments as 16-byte pieces: half h of the wave takes floats [4h, 4h + 4) of an 8-wide K chunk, MFMA j of the chunk
// uses element j on both operands -- which k a (half, j) pair stands for is immaterial as long as A and B agree.
#pragma once
#include "k_yolo.h"

typedef float sd_f4 __attribute__((ext_vector_type(4)));

struct SdConvArgsF {
    const float* in; const float* wgt; const float* bias; const float* res; float* out;
    const float* zero;       // >= 16 zero bytes: the source of padded taps and of rows beyond the last pixel
    int N, H, W, cin, cinStride;
    int Ho, Wo, cout, outStride, resStride;
    int ksize, stride, pad, leaky;
    int pair;                // first layer: the input has 4 channels per pixel and K step s holds taps 2 s and 2 s + 1 (tap 9 = zeros):
                             // 5 steps of 8 instead of 9 steps of 8 with five zero channels each; weights [coutPad][5][2][4].  k_conv_f32<8, ...> IS
                             // this form and is launched for the first layer alone (yolo_plan_launch): the kernel does not test the flag
    int tilesX, tilesY, groupY;      // pixel tiles, filter tiles (groupY divides tilesY): the launch is 1-D, SD_F32_GRID(tilesX, tilesY) workgroups
    // k_conv_f32's set-up, computed where the struct is filled (yolo_f32_setup, sd_yolo_plan.h): the kernel divides by multiply-high
    // (sd_udiv below) and moves its gather pointers from tap to tap by adding one of two byte distances
    unsigned mHoWo, sHoWo, mWo, sWo;              // n / (Ho Wo), n / Wo
    unsigned mPerGroup, sPerGroup, mGroupY, sGroupY;      // n / (ceil8(tilesX) / 8 * groupY), n / groupY
    int tapCol, tapRow;              // bytes from a tap's first channel to the next tap's: one column on, (kw = ksize - 1 ->) first column of the next row
};

// n / d for n < 2^31 with the pair (m, s) sd_magic_div(d) made on the host (sd_yolo_plan.h)
__device__ __forceinline__ unsigned sd_udiv(unsigned n, unsigned m, unsigned s) { return (__umulhi(n, m) + n) >> s; }

// The element-wise tail of the epilogue on one 16-byte piece: x = acc + bias, leaky ReLU, + shortcut, in that order, on PAIRS of floats
// (v_pk_add_f32 / v_pk_mul_f32: half the instructions of the add, the multiply and the shortcut add).  The leaky ReLU is max(x, slope x) with
// slope 0.1 -- for every finite x, +-0 included, the value of x > 0 ? x : 0.1 x -- and slope 1 on a linear layer (x 1 and max(x, x) leave x
// as it is): no compare, no select, no branch on `leaky`.  -ffp-contract=off: no FMA forms.  An `inside` epilogue spends 160 VALU instructions on
// its 64 outputs per lane instead of 320.  Measured alone (the set-up below in both builds, alternating runs on one box): headline 1109.3 ->
// 1110.9 frames/s, + 0.13 %, the same sign in every pair of runs but no larger than the parent's own spread; results bit for bit the same.
typedef float sd_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ sd_f4 sd_f32_tail(const sd_f4 a, const sd_f4 b, const float slope, const sd_f4 r, const bool res)
{
    sd_f2 x0 = a.xy + b.xy, x1 = a.zw + b.zw;
    x0 = __builtin_elementwise_max(x0, x0 * slope); x1 = __builtin_elementwise_max(x1, x1 * slope);
    if (res) { x0 += r.xy; x1 += r.zw; }
    return sd_f4{x0.x, x0.y, x1.x, x1.y};
}

// Where a K step's staging instructions go among its MFMAs (LLVM's sched_group_barrier: "next, N instructions of this class", in the order the
// groups are written).  The step is one basic block of TM MFMAs behind the R0 fragment reads of its first K chunk.  Behind MFMA g:
//   g < ceil(RD / 2)              two of the RD fragment reads of the step's later K chunks (needed from MFMA TM / 2 on);
//   g = W0, W0 + WS, ...          one of the NS ds_write_b128 of the next stage;
//   g = L0, L0 + LS, ...          one of the NS buffer_load_dwordx4 of the stage after it, alone: its address walks in scalar registers (load i
//                                 overwrites the registers write i read: every write stands in front of every load);
//   every other gap               nothing: what is left (lgkmcnt / vmcnt waits, scalar instructions) falls where the scheduler likes.
// No gap holds more than one vector-memory or two LDS instructions: tools/conv_f32_loop_gaps.py prints the emitted gaps,
// tests/test_conv_f32_loop_schedule.py pins them.  WHERE the gaps lie matters far more than that they are apart -- measured on the 128-filter
// tile (headline, frames/s, builds alternated with the parent on one box; TM = 32, writes / loads behind MFMA ...):
//   2, 3, ..., 9 alternating (write, load, write, ...)           - 14.8 %      10 - 17 alternating   - 7.4 %      16 - 23 alternating   - 2.7 %
//   6, 8, ..., 20 alternating                                    -  3.6 %      2, 5, ..., 23 alternating  + 0.2 %   6, 9, ..., 27 alternating  + 1.2 %
//   writes 6, 9, 12, 15, loads 18, 21, 24, 27                    +  1.6 %      writes 4, 8, 12, 16, loads 20, 23, 26, 29 (this)  + 1.8 %
//   writes 4, 7, 10, 13, loads 16 - 25   + 0.9 %;   writes 6 - 15, loads 24, 25, 26, 27   + 0.9 %;   writes 3, 7, 11, 15, loads 19, 23, 27, 31   + 0.9 %
// (the parent's own spread in those sessions: 0.02 - 0.34 %; profiles/conv_f32_schedule_bench.json).  What the numbers say: a staging instruction
// directly behind the post-barrier burst of fragment reads, or directly behind another one, stalls its wave at issue (instruction issue is in
// order: the MFMAs behind it wait with it); a load two or three MFMAs behind the write whose registers it overwrites is the worst case; writes
// early, loads late, each three or four MFMAs apart is the best found.
template <int TM, int R0, int RD, int NS, int W0, int WS, int L0, int LS, int G = 0>
__device__ __forceinline__ void sd_f32_place()
{
    static_assert(W0 >= (RD + 1) / 2 && W0 + WS * (NS - 1) < L0 && L0 + LS * (NS - 1) < TM, "the step's staging does not fit its MFMA gaps");
    if constexpr (G == 0) __builtin_amdgcn_sched_group_barrier(0x100, R0, 0);               // the first chunk's R0 fragment reads, behind the barrier
    if constexpr (G < TM) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                  // one MFMA
        if constexpr (2 * G < RD) __builtin_amdgcn_sched_group_barrier(0x100, RD - 2 * G < 2 ? RD - 2 * G : 2, 0);      // DS reads
        else if constexpr (G >= W0 && (G - W0) % WS == 0 && (G - W0) / WS < NS) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);      // one DS write
        else if constexpr (G >= L0 && (G - L0) % LS == 0 && (G - L0) / LS < NS) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // one VMEM read, alone
        sd_f32_place<TM, R0, RD, NS, W0, WS, L0, LS, G + 1>();
    }
}

// Tile shapes: WM waves along the filters x (NW / WM) waves along the pixels, a wave owns MT x 2 MFMA tiles (32 MT filters x 64
// pixels), K steps of BK channels.  Four instantiations exist, all launched by the one layer walk of sd_yolo_api.hip as yolo_plan_launch
// (sd_yolo_plan.h) chooses them, in the f32-class modes for every convolution their Winograd / bf16-limb kernels do not take:
//   <16, 2, 2, 4>   128 filters x 128 pixels, three workgroups per CU: every layer with more than 64 filters
//   <16, 1, 2, 4>    64 filters x 256 pixels: the layers with 33 - 64 filters
//   <16, 1, 1, 4>    32 filters x 256 pixels: the layers with <= 32 filters -- either would waste half or three quarters of a 128-filter tile
//   <8, 1, 1, 8>     32 filters x 512 pixels on 8 waves: the first layer (3 input channels in `pair` mode)
// The measurements against the tiles tried and dropped (8-wave 128 x 256, 32-channel steps, 8-wave small tiles): DESIGN.md 4.1.
// LDS holds TWO stages: while the MFMAs of stage s run, the tiles of stage s + 1 (fetched into registers one
// step earlier) are written to the other buffer and the global loads of stage s + 2 are issued -- one barrier per step, and
// neither the address arithmetic of the gather nor the LDS writes sit between two barriers with the MFMA pipe idle.  Behind the two
// stages lie the tile's BM bias floats (SD_F32_LDS counts them), written once by the prologue and read by the epilogue.
template <int BK, int WM, int MT, int NW>
__global__ void __launch_bounds__(64 * NW, NW == 8 ? 1 : (WM == 2 && BK == 16 ? 3 : 2)) k_conv_f32(SdConvArgsF A)
{
    constexpr int NT = 64 * NW;                         // NW = 8: one workgroup per CU; NW = 4: two independent workgroups per CU
    constexpr int WN = NW / WM, BM = 32 * MT * WM, BN = 64 * WN;
    constexpr int LD = BK + 4;                          // LDS row length in floats (16-byte aligned rows, 2-way conflicts at worst)
    constexpr int CPR = BK / 4;                         // 16-byte chunks per row
    constexpr int XC = (BN * CPR + NT - 1) / NT;        // activation chunks per thread per step
    constexpr int WC = (BM * CPR + NT - 1) / NT;
    constexpr int STAGE = (BM + BN) * LD;               // floats per stage
    constexpr int NCH = BK / 8;                         // 8-wide K chunks per step
    extern __shared__ __align__(16) float smemf[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, h = lane >> 5;
    const int wm = wv % WM, wn = wv / WM;               // wave tile: filters [32 MT wm, +32 MT), pixels [64 wn, +64)
    // Every argument the set-up needs is read here, ahead of any branch: the compiler fetches them with a few wide scalar loads and one wait.
    const float* const in = A.in; const float* const wgt = A.wgt; const float* const zero = A.zero;
    const int H = A.H, W = A.W, cin = A.cin, cinStride = A.cinStride, Ho = A.Ho, Wo = A.Wo, ksize = A.ksize, stride = A.stride, pad = A.pad;
    const int tilesX = A.tilesX, groupY = A.groupY;
    const int N = A.N, HoWo = Ho * Wo, npix = N * HoWo;
    const unsigned mHoWo = A.mHoWo, sHoWo = A.sHoWo, mWo = A.mWo, sWo = A.sWo;
    const ptrdiff_t tapCol = A.tapCol, tapRow = A.tapRow;
    const float slope = A.leaky ? 0.1f : 1.f;
    // XCD-aware order (workgroup L runs on XCD L % 8, each XCD has its own 4 MB L2): XCD x owns a CONTIGUOUS range of pixel tiles (the
    // rows that neighbouring pixel tiles share for the 3 x 3 taps meet in one L2) and walks it once per GROUP of groupY filter tiles,
    // the filter tiles of a group back to back on each pixel tile.  groupY is chosen on the host so that a group's weights stay
    // L2-resident (<= 2.5 MB): the activations are then fetched from HBM tilesY / groupY times instead of tilesY times, without
    // trading them for weight misses (all 8 filter tiles of a 512 -> 1024 3 x 3 layer are 19 MB of weights).  Measured per 128-image batch
    // (FETCH_SIZE, doubled): 246 GB read in plain (pixel tile, filter tile) grid order, 139 GB with this order at the same 124.1 ms;
    // all filter tiles back to back regardless of their weights: 103 GB but 126.4 ms.
    const int perXcd = (tilesX + 7) >> 3;
    const unsigned slot = blockIdx.x >> 3, perGroup = perXcd * groupY;
    const unsigned grp = sd_udiv(slot, A.mPerGroup, A.sPerGroup), r = slot - grp * perGroup, rq = sd_udiv(r, A.mGroupY, A.sGroupY);
    const int tx = (blockIdx.x & 7) * perXcd + rq, ty = grp * groupY + (r - rq * groupY);
    if (tx >= tilesX) return;
    const int pix0 = tx * BN, co0 = ty * BM;
    const int taps = ksize * ksize;                     // 1 or 9 (yolo_plan_net admits no other size): the tap masks below hold ksize <= 3
    constexpr bool pair = BK == 8;                      // the 8-channel step exists for the first layer alone (yolo_plan_launch), in its tap-pair form (SdConvArgsF::pair)
    __builtin_assume(pair || cin >= 2 * BK);            // stored input channels are a multiple of 32 (yolo_plan_net): the first request never ends a tap
    const int ksteps = pair ? (taps + 1) / 2 : taps * (cin / BK);
    const int wrow = pair ? 8 * ksteps : taps * cin;    // floats per filter
    sd_f16v acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
    // (The two 32-filter tiles; the 128- and 64-filter tiles took this form one step further: "The scalar walk" below.  The one-time (y, x)
    // arithmetic and the tap masks are common to all four.)  Staging addresses are kept as running pointers: inside a filter tap a step only adds BK floats to each of them.  The im2col gather's
    // (y, x) arithmetic and bounds tests run ONCE, here: per activation chunk a thread keeps xtrue, the address its piece would have if every
    // tap lay inside the image (64-bit: the first layers' tensors exceed 2^31 elements at batch 256; outside the image it is formed and never
    // dereferenced), and tapmask, bit t = tap t of this pixel is inside the image (and the pixel exists).  A tap change (every cin / BK steps)
    // adds a uniform byte distance to xtrue -- tapCol, or tapRow behind a row's last tap -- and selects xptr = bit ? xtrue : the zero page,
    // xinc = bit ? BK : 0: one 64-bit add, one bit test and three selects per chunk, no multiply, no branch on exec, no argument reload.  (The per-step form of
    // the gather arithmetic, ~150 VALU instructions with 64-bit multiplies and branches, cost the MFMA pipe a quarter of its time:
    // tools/micro/conv_loop_cost.hip; the per-tap form this replaces compiled to nested exec-mask branches around two 64-bit and two 32-bit
    // multiplies per pointer, five copies of it in the kernel.)  Static counts per wave of the 128-filter tile, before -> after: 377 -> 163 VALU
    // instructions before the first barrier, 60 -> 8 of them integer multiplies, 16 -> 0 integer multiplies between the first and the last MFMA
    // (profiles/conv_f32_setup_isa.txt, pinned by tests/test_conv_f32_isa_budget.py).  Measured, alternating runs on one box, in steps: the tap
    // pointers with plain divisions in the set-up, headline 1096.1 -> 1108.0 frames/s (+ 1.1 %, parent spread 0.3 %) and 118.0 -> 116.6 ms per
    // 128-image detector pass; the divisions by multiply-high on top, 1108.0 -> 1109.3 (+ 0.1 %: inside the spread; kept because they are what
    // brings the set-up below half the parent's instructions); the packed epilogue on top: sd_f32_tail.  Results bit for bit the parent's
    // (tests/test_gpu_conv_f32_epilogue.py, tests/test_gpu_conv_f32_setup.py).
    // The pixel of chunk 0 is split into (image, row, column) by two multiply-highs (sd_udiv); chunk i + 1 lies NT / CPR pixels further on and
    // follows from chunk i by adding the (uniform) split of that distance with carries.
    // DEEP: two register sets, a stage's tiles are requested TWO steps before they go to LDS.  The 64-filter tile <.., 1, 2, ..> stages
    // four activation chunks per thread; with running pointers a second set would have cost it its third wave per SIMD (186 VGPRs).  With the
    // scalar walk it fits (166 VGPRs at __launch_bounds__(256, 3)); measured with its step placed like the 128-filter tile's (writes behind
    // MFMAs 4, 7, ..., 16, loads behind 19, 22, ..., 31), bit-identical: headline 1150.8 -> 1150.3 frames/s, nothing -- not kept
    // (profiles/conv_f32_walk_bench.json).
    constexpr bool DEEP = !(WM == 1 && MT == 2);
    constexpr int NSET = DEEP ? 2 : 1;
    // ALWAYS: every K step writes a stage and requests one, whether or not the tile has one left (see request() below) -- the tiles whose weight rows
    // fill their threads.  The two 32-filter tiles store their weight rows under an exec-mask branch, which splits the step anyway, and measured
    // slower with unconditional requests (first layer + 12.6 %, the 1 x 1 64 -> 32 layer + 2.5 %): they keep the conditional store and request, inside
    // the step.  The end-of-tile handling in retap() is the same for all tiles; on these two no request follows it.
    constexpr bool ALWAYS = WC * NT == BM * CPR;
    static_assert(XC * NT == BN * CPR && NT % CPR == 0, "every thread stages XC activation chunks, all of them the same piece of their rows");
    // The scalar walk (ALWAYS tiles).  Everything a staging address does during a tile is wave-uniform -- a step adds BK floats to every live
    // pointer, a tap change the same tapCol / tapRow to every lane -- so these two tiles do not keep pointers at all.  They stage with buffer
    // loads, address = descriptor base + voffset (VGPR) + soffset (SGPR):
    //   two descriptors per workgroup, built from kernel arguments and blockIdx-derived values only (uniform to the compiler: no waterfall loop,
    //   no v_readfirstlane), stride 0.  Weights: base = the tile's first filter row, records = its BM rows.  Activations: base = the tile's
    //   ANCHOR, tap (0, 0), channel 0 of pixel pix0, formed in 64 bits (it lies in front of the tensor by the padding at an image's corner;
    //   no live lane reads there), records = SD_F32_WALK_RECORDS = 2^31 bytes;
    //   per lane, fixed for the tile: woff[i] = (filter row) wrow 4 + 16 q; xoff[i] = (chunk's tap-(0, 0) pixel - anchor pixel) 4 cinStride + 16 q, in
    //   [0, 2^31) for every live chunk (the host refuses a layer where it could not be: yolo_f32_walk_fits, sd_yolo_plan.h); tapmask[i] as before;
    //   the walk: wsoff and xsoff, one SGPR each.  request() adds 4 BK bytes to both with scalar adds; a tap change adds tapCol - 4 cin (tapRow -
    //   4 cin behind a row's last tap) to xsoff -- xsoff is then the byte distance from tap (0, 0) to the current (tap, channel), never negative --
    //   and, per activation chunk, ONE bit test and ONE select: xv[i] = bit ? xoff[i] : SD_F32_WALK_SENTINEL.  The sentinel lies outside the
    //   records whatever the scalar offset adds: the range check answers a padded tap (and a chunk beyond the last pixel) with zeros and touches
    //   no memory -- the zero page is not read;
    //   the tile's end (`dead` in retap(), as before): both record counts become 0 by scalar selects, so the 1 + NSET requests behind the last
    //   stage read nothing whatever their offsets are.  Requests stay unconditional, waits counted, the step one basic block.
    // The loads, their order and the LDS map are the parent's: results bit for bit the same (tests/test_gpu_conv_f32_scalar_walk.py); the address
    // arithmetic is walked on the host for every tile, chunk, tap and step of the detector's layers (tests/cpp/conv_f32_offsets_check.cpp).
    // Static counts, VALU per loop step with its tap-change block, before -> after: 24 -> 6 on the 128-filter tile, 39 -> 12 on the 64-filter tile;
    // none between a step's first and last MFMA (tests/test_conv_f32_scalar_walk.py).  What was measured: DESIGN.md 4.1, "The scalar walk".
    // The two 32-filter tiles keep the pointers below, the zero page and their conditional request.
    sd_f4 xr[NSET][XC], wr[NSET][WC];
    const float* wptr[WC];
    const float* xptr[XC];
    const char* xtrue[XC];
    unsigned tapmask[XC];
    int winc[WC], xinc[XC];
    // ALWAYS tiles: see "The scalar walk" below.  Per lane: woff / xoff (fixed for the tile) and xv, the activations' voffset of the current tap
    unsigned woff[WC], xoff[XC], xv[XC];
    const char* wbase = nullptr; const char* xbase = nullptr;      // the two descriptors' bases (uniform)
    int wrec = 0, xrec = 0;                             // their record counts: 0 from the tile's end on
    int wsoff = 0, xsoff = 0;                           // the walk: one scalar byte offset per descriptor
    const int q = tid % CPR;                            // this thread's 16-byte piece of a row, the same in all its chunks
    {
        constexpr unsigned D = NT / CPR;                // pixels between two chunks of a thread
        const unsigned dn = sd_udiv(D, mHoWo, sHoWo), dr = D - dn * HoWo, dy = sd_udiv(dr, mWo, sWo), dx = dr - dy * Wo;
        const unsigned p = pix0 + tid / CPR;
        unsigned n = sd_udiv(p, mHoWo, sHoWo);
        const unsigned pr = p - n * HoWo;
        unsigned yo = sd_udiv(pr, mWo, sWo), xo = pr - yo * Wo;
        const unsigned rowrep = ksize == 1 ? 1u : 1u | 1u << ksize | 1u << 2 * ksize;      // bit 0 of every filter row
        const unsigned rowlow = (1u << ksize) - 1u;
        int pixelA = 0;                                 // ALWAYS: the anchor's pixel index, tap (0, 0) of pixel pix0 (scalar; negative by the padding at an image's corner)
        if constexpr (ALWAYS) {
            const unsigned n0 = sd_udiv((unsigned)pix0, mHoWo, sHoWo), pr0 = pix0 - n0 * HoWo, y0 = sd_udiv(pr0, mWo, sWo), x0 = pr0 - y0 * Wo;
            pixelA = ((int)(n0 * H) + ((int)y0 * stride - pad)) * W + ((int)x0 * stride - pad);
            xbase = (const char*)in + (long long)pixelA * (4 * cinStride);
            xrec = (int)SD_F32_WALK_RECORDS;
        }
#pragma unroll
        for (int i = 0; i < XC; i++) {
            if (i > 0) {
                xo += dx; const bool cx = xo >= (unsigned)Wo; xo -= cx ? Wo : 0;
                yo += dy + (cx ? 1 : 0); const bool cy = yo >= (unsigned)Ho; yo -= cy ? Ho : 0;
                n += dn + (cy ? 1 : 0);
            }
            const int yi = __mul24((int)yo, stride) - pad, xi = __mul24((int)xo, stride) - pad;      // tap (0, 0) of the pixel
            // taps k of an axis inside the map: l <= k < h with l = max(-c, 0), h = min(extent - c, ksize), c the coordinate of tap 0.  pad <= 1, so
            // l is 0 or 1 and h >= 1: the columns' bits are (1 << h) - 1 - l, repeated per filter row (x rowrep, bit 0 of every row), and the
            // rows' bits [l ksize, h ksize) are (1 << h ksize) - 1 - l rowlow (rowlow: the first row's bits)
            const int lx = max(-xi, 0), hx = min(W - xi, ksize), ly = max(-yi, 0), hy = min(H - yi, ksize);
            const unsigned mk = __umul24((1u << hx) - 1u - lx, rowrep) & ((1u << __umul24(hy, ksize)) - (1u + __umul24(ly, rowlow)));
            // piece q of a row: channels [4 q, +4) of the tap -- in `pair` mode tap 2 s + q of K step s, all four channels of its pixel.  A chunk beyond the
            // last pixel lies in an image >= N
            tapmask[i] = n < (unsigned)N ? (pair ? mk >> q : mk) : 0;
            // 32-bit pixel index, 24-bit factors (the host refuses larger inputs); the byte offset is 64-bit
            const int pixel = __mul24((int)__umul24(n, H) + yi, W) + xi;
            if constexpr (ALWAYS) xoff[i] = (unsigned)(pixel - pixelA) * (unsigned)(4 * cinStride) + 16u * q;      // live chunks: in [0, 2^31) (yolo_f32_walk_fits)
            else xtrue[i] = (const char*)in + ((long long)pixel * (4 * cinStride) + (pair ? 4 * cinStride : 16) * q);
        }
    }
    {
        constexpr int DW = NT / CPR;                    // filters between two chunks of a thread
        // the tile's first filter row in scalar registers; a thread's own row and piece within the tile: a 32-bit byte offset
        if constexpr (ALWAYS) {
            wbase = (const char*)(wgt + (size_t)co0 * (unsigned)wrow);
            wrec = BM * wrow * 4;                       // the tile's BM filter rows (weight rows are padded to the widest filter tile: all of them exist)
#pragma unroll
            for (int i = 0; i < WC; i++) woff[i] = __umul24(tid / CPR + DW * i, wrow) * 4u + 16u * q;
        } else {
            const char* const w0 = (const char*)(wgt + (size_t)co0 * (unsigned)wrow) + (__umul24(tid / CPR, wrow) * 4u + 16u * q);
#pragma unroll
            for (int i = 0; i < WC; i++) {
                const bool on = (WC * NT == BM * CPR) || tid + NT * i < BM * CPR;
                wptr[i] = on ? (const float*)(w0 + (size_t)(4 * DW * i) * (unsigned)wrow) : zero;
                winc[i] = on ? BK : 0;                  // (tap, channel) is one contiguous axis of a filter's weights
            }
        }
    }
    int nreq = 0;                                       // stages requested so far
    int c0 = 0, kw = 0, pdx = q;                        // pdx (`pair`): the column of this thread's tap in its filter row
    unsigned tapbit = 1;                                // the current tap's bit in tapmask (`pair`: the bit of tap 2 s at K step s, tapmask is shifted by q)
    auto select = [&]() {
#pragma unroll
        for (int i = 0; i < XC; i++) {
            const bool ok = (tapmask[i] & tapbit) != 0;
            if constexpr (ALWAYS) xv[i] = ok ? xoff[i] : SD_F32_WALK_SENTINEL;
            else {
                xptr[i] = ok ? (const float*)xtrue[i] : zero;
                xinc[i] = ok && !pair ? BK : 0;
            }
        }
    };
    auto retap = [&]() {                                // the next tap (`pair`: the next two)
        if (pair) {
            // a thread's tap goes two columns on; past the row's end (once at most: ksize >= 2 wherever a second step exists) it wraps into the next row
            pdx += 2;
            const bool wrap = pdx >= ksize;
            pdx -= wrap ? ksize : 0;
            const ptrdiff_t d = wrap ? tapRow + tapCol : 2 * tapCol;
#pragma unroll
            for (int i = 0; i < XC; i++) xtrue[i] += d;
            tapbit <<= 2;
        } else {
            kw++;
            const bool wrap = kw == ksize;
            if (wrap) kw = 0;
            if constexpr (ALWAYS) xsoff += (int)(wrap ? tapRow : tapCol) - 4 * cin;      // request() has walked the tap's cin channels
            else {
                const ptrdiff_t d = wrap ? tapRow : tapCol;
#pragma unroll
                for (int i = 0; i < XC; i++) xtrue[i] += d;
            }
            tapbit <<= 1;
        }
        select();
        const bool dead = nreq >= ksteps;               // the tile has no stage left to request: see request() below
        if constexpr (ALWAYS) { wrec = dead ? 0 : wrec; xrec = dead ? 0 : xrec; }
        else {
#pragma unroll
            for (int i = 0; i < WC; i++) { wptr[i] = dead ? zero : wptr[i]; winc[i] = dead ? 0 : winc[i]; }
        }
    };
    select();
    // A stage's request is split in two.  request(): its loads and the walk's two scalar adds (the pointers' post-increments on the 32-filter tiles), straight-line -- on the ALWAYS tiles issued by
    // EVERY K step and 1 + NSET times by the prologue, whether or not the tile has a stage left to ask for.  advance(): the tap walk behind it, with
    // its one branch, placed where it splits no MFMA sequence: behind a step's last MFMA, in front of its barrier.
    // Why unconditional: with `if (stage left) fetch` inside the step the compiler had to assume, at every ds_write, that the younger register
    // set's loads might not have been issued, and waited with vmcnt(3..0) -- for loads requested ONE step earlier; DEEP's two-step distance was in the
    // registers but not in the waits.  With every request always issued the waits are counted (vmcnt(7) on the 128-filter tile), and the step
    // between its first and its last MFMA is one basic block whose instructions can be placed (sd_f32_place).
    // What a request behind the tile's last stage reads: nothing.  The tile's last real request ends its last tap, so the retap() behind it is
    // where the tile ends (`dead`, wave-uniform: nreq >= ksteps; it stays set for the 1 + NSET requests that follow, one per remaining step): it
    // sets both descriptors' record counts to zero, every lane of every later load is out of range and gets zeros, into a register set that goes
    // to an LDS buffer no MFMA reads again.  No load reaches an address the parent did not read:
    //   weights       woff + wsoff walks [tap][channel] of the lane's filter row contiguously; behind the last real request wsoff stands one step
    //                 past the row: the dead retap() has emptied the descriptor before the next load;
    //   activations   a live lane's address is anchor + xoff + xsoff = the parent's xtrue + channel offset exactly; behind the tile's end xsoff
    //                 keeps walking under the empty descriptor;
    //   padded taps   select() gives SD_F32_WALK_SENTINEL while the tap's mask bit is clear: beyond the records, zeros from the range check;
    //   chunks beyond npix   tapmask == 0: the sentinel at every tap, from the first request on.
    // retap() moves scalar registers, one VALU select per activation chunk and nothing else: no path of the loop issues a load another does not,
    // which is what keeps the waits counted.  (On a tile that is not ALWAYS -- the two 32-filter tiles, whose requests are conditional -- padded
    // taps, chunks beyond npix and absent weight rows read the zero page A.zero through pointers with increment 0.)
    auto request = [&](const int set) {
        if constexpr (ALWAYS) {
            const __amdgpu_buffer_rsrc_t dw = __builtin_amdgcn_make_buffer_rsrc((void*)wbase, 0, wrec, 0x00020000);
            const __amdgpu_buffer_rsrc_t dx = __builtin_amdgcn_make_buffer_rsrc((void*)xbase, 0, xrec, 0x00020000);
#pragma unroll
            for (int i = 0; i < WC; i++) wr[set][i] = __builtin_bit_cast(sd_f4, __builtin_amdgcn_raw_buffer_load_b128(dw, (int)woff[i], wsoff, 0));
#pragma unroll
            for (int i = 0; i < XC; i++) xr[set][i] = __builtin_bit_cast(sd_f4, __builtin_amdgcn_raw_buffer_load_b128(dx, (int)xv[i], xsoff, 0));
            wsoff += 4 * BK; xsoff += 4 * BK;
        } else {
#pragma unroll
            for (int i = 0; i < WC; i++) { wr[set][i] = *(const sd_f4*)wptr[i]; wptr[i] += winc[i]; }
#pragma unroll
            for (int i = 0; i < XC; i++) { xr[set][i] = *(const sd_f4*)xptr[i]; xptr[i] += xinc[i]; }
        }
    };
    auto advance = [&]() {
        nreq++;
        if (pair) { retap(); return; }
        c0 += BK;
        if (c0 == cin) { c0 = 0; retap(); }
    };
    auto store = [&](int buf, const int set) {
        float* sW = smemf + buf * STAGE;
        float* sX = sW + BM * LD;
#pragma unroll
        for (int i = 0; i < WC; i++) { const int chunk = tid + NT * i; if ((WC * NT == BM * CPR) || chunk < BM * CPR) *(sd_f4*)(sW + (chunk / CPR) * LD + 4 * (chunk % CPR)) = wr[set][i]; }
#pragma unroll
        for (int i = 0; i < XC; i++) { const int chunk = tid + NT * i; if ((XC * NT == BN * CPR) || chunk < BN * CPR) *(sd_f4*)(sX + (chunk / CPR) * LD + 4 * (chunk % CPR)) = xr[set][i]; }
    };
    const int aoff = (32 * MT * wm + r32) * LD + 4 * h, boff = BM * LD + (64 * wn + r32) * LD + 4 * h;
    sd_f4 fa[2][MT], fb[2][2];                          // fragments of two consecutive K chunks: the reads of chunk c + 1 are issued before the MFMAs of chunk c
    auto frags = [&](int buf, int kc, int slot) {
        const float* base = smemf + buf * STAGE;
#pragma unroll
        for (int m = 0; m < MT; m++) fa[slot][m] = *(const sd_f4*)(base + aoff + 32 * m * LD + 8 * kc);
#pragma unroll
        for (int n = 0; n < 2; n++) fb[slot][n] = *(const sd_f4*)(base + boff + 32 * n * LD + 8 * kc);
    };
    auto mfmas = [&](int slot) {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int n = 0; n < 2; n++)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[slot][m][j], fb[slot][n][j], acc[m][n], 0, 0, 0);
    };
    // The two waves that share a SIMD (w and w + 4) do their staging at DIFFERENT K chunks of a step: the ~150 address / LDS-write
    // instructions of one wave then run under the other wave's MFMAs instead of both leaving the MFMA pipe idle together.
    const int myslot = NW == 8 ? (NCH >= 4 ? 2 * (wv >> 2) : (NCH == 2 ? (wv >> 2) : 0)) : 0;
    // DEEP: stage s lives in register set s & 1 from its request (two steps ahead: ~12 000 cycles with three waves per SIMD, against an
    // L2 / HBM latency of several thousand under load -- with ONE step of distance the ds_writes waited on their loads for 11 % of
    // the kernel time) until it is written to LDS buffer s & 1 during step s - 1.  (Until the requests became unconditional that distance was
    // in the registers only: the waits in front of the ds_writes were vmcnt(3..0), which also waits for the loads issued one step earlier.)
    // The tile's BM bias floats are staged in LDS behind the two stages (requested first, written with stage 0): the epilogue reads them with
    // ds_read_b128, which counts in lgkmcnt -- a bias load from global memory there shares vmcnt with the tile's stores and made every
    // store wait for the one before it (see the epilogue).
    float* const sBias = smemf + 2 * STAGE;
    // every thread requests a piece (no branch, no zero fill; the first BM / 4 threads write theirs); bias rows are padded to the widest filter tile
    // (coutPad): no test against cout
    const sd_f4 bq = *(const sd_f4*)(A.bias + co0 + 4 * (tid % (BM / 4)));
    // The order below exposes two latencies (stage 1 is requested only behind store(0, 0)'s wait).  Requesting stages 0 AND 1 before the first
    // wait was measured and is not kept: headline 1085.2 / 1086.2 frames/s against 1087.0 / 1087.4 with this order in alternating runs on
    // one box, per-layer fixed cost the same (profiles/conv_f32_epilogue_layers_steps.txt) -- the two other workgroups of the CU cover it.
    // Every tile has at least two K steps (32 stored channels = two 16-channel steps; the first layer's nine taps = five): stage 1 always exists,
    // stage 2 is all zeros on a two-step tile (advance() behind stage 1 was the tile's last real request).
    request(0); advance();
    store(0, 0);
    if (tid < BM / 4) *(sd_f4*)(sBias + 4 * tid) = bq;
    request(NSET - 1); advance();
    if (DEEP && (ALWAYS || ksteps > 2)) { request(0); advance(); }
    __syncthreads();
    // Measured around this loop at batch 128 (ms per detector batch; the ablation builds -- no barrier / no staging / no fragment reads -- gave wrong results, existed for timing only and are no longer in this source):
    // as is 121.0-122.5; without the barrier -1 % (122.9 against 124.1, measured before the two-step prefetch); without any staging (no
    // loads, no LDS writes, no address updates) 109.3; staging without the
    // global loads 120.1 -- i.e. what the staging costs is not the memory latency.  Requests issued unconditionally (so that the
    // compiler can wait with vmcnt(7..4) instead of vmcnt(3..0)) 122.2 (neutral then; with the whole step straight-line and the compiler's own
    // order it is - 3.2 % on the headline, PLACED it is + 1.1 ... + 1.8 %: sd_f32_place above); a staging map whose ds_write_b128 passes hit 16 distinct bank
    // quads (SQ_LDS_BANK_CONFLICT 0 instead of 33 % of the LDS-active cycles, but the LDS is busy only 10-16 % of the time) 123.7; the
    // barrier moved in front of the step's last chunk with the next step's first fragments requested right behind it (the post-barrier
    // LDS round trip under 16 MFMAs) 121.4.  The same tile staged entirely by LDS-DMA (global_load_lds_dwordx4 into unpadded, XOR-
    // swizzled rows, a ring of three 16 KB stages at three workgroups per CU, counted vmcnt(4) + one barrier per step; results
    // identical) 132.6 against 120.3: slower, not kept.  The weight operand kept out of LDS altogether (each lane fetches its own A
    // fragments from L2 one step ahead, only the activations are staged: half the LDS writes and reads; results identical) 136.0
    // against 119.7: slower, not kept -- so the ~9 % that vanish with the staging are not the LDS writes as such.  s_setprio 1 / 3 around every MFMA cluster (round 4): 117.7 / 117.6
    // and 118.0 / 118.0 against 118.1 and 118.0 -- nothing.  PMC: clock 2.37-2.39 GHz in these kernels (no DVFS give-back), MFMA pipe busy
    // 83 % in the 3 x 3 body layers.
    auto step = [&](const int ks, const int par) {     // par = ks & 1, a literal at both call sites
        const int cur = par;
        frags(cur, 0, 0);
#pragma unroll
        for (int kc = 0; kc < NCH; kc++) {
            if (kc + 1 < NCH) frags(cur, kc + 1, (kc + 1) & 1);
            mfmas(kc & 1);
            if (kc == myslot) {                         // stage ks + 1 into the other buffer, stage ks + 1 + NSET requested into the set that frees
                if constexpr (ALWAYS) {
                    store(cur ^ 1, DEEP ? par ^ 1 : 0); // the tile's last step writes a set of zeros into the buffer nobody reads again
                    request(DEEP ? par ^ 1 : 0);
                } else {
                    if (ks + 1 < ksteps) store(cur ^ 1, DEEP ? par ^ 1 : 0);
                    if (ks + 1 + NSET < ksteps) { request(DEEP ? par ^ 1 : 0); advance(); }
                }
            }
        }
        // The 128-filter tile's staging is placed among its MFMAs (sd_f32_place: the measurements are there).  The 64-filter tile keeps the
        // compiler's order: it has one register set (a load placed late would not be back for its write early in the next step).
        if constexpr (BK == 16 && WM == 2 && MT == 2) sd_f32_place<NCH * 8 * MT, MT + 2, (NCH - 1) * (MT + 2), WC + XC, 4, 4, 20, 3>();
        if constexpr (ALWAYS) advance();
        // The barrier stays BEHIND the step's last MFMA: hoisted above them (legal, they touch no memory) the two waves of a SIMD
        // would reach it a staging block apart and the earlier one would sit there with its remaining MFMAs unissued.
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
    };
    int ks = 0;
    for (; ks + 1 < ksteps; ks += 2) { step(ks, 0); step(ks + 1, 1); }
    if (ks < ksteps) step(ks, 0);
    if constexpr (WM == 1) {
        // ---- epilogue.  D column = pixel (lane & 31), rows = filters (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): written straight from the
        // accumulators a store instruction would cover 32 pixels x 32 bytes.  The wave's 32-pixel half tiles go through its own piece of
        // the (now free) LDS instead -- [pixel][32 MT filters] -- and come back with consecutive lanes on consecutive 16-byte pieces of a
        // pixel's filter row: stores and shortcut reads of 128 / 256 contiguous bytes per pixel.  (The first layers write 5 GB per
        // 128-image batch against a few dozen K steps: their time was the scattered stores.)  Only the <= 64-filter tiles (WM == 1) do
        // this: on the 128-filter tiles, whose epilogue is 3 % of a long K loop and overlaps the other workgroups' MFMAs, the LDS round
        // trip made every 3 x 3 body layer 1-6 % slower (measured), so they keep the direct stores below.
        constexpr int TWD = 32 * MT, TLD = TWD + 4;           // floats per pixel row of the transpose tile (+4: rows 16 bytes apart mod 256)
        constexpr int PPI = 64 / (TWD / 4);                   // pixels per store instruction: a pixel row is TWD / 4 pieces
        static_assert(NW * 32 * TLD <= 2 * STAGE, "the transpose tiles of the epilogue must fit the staging buffers");
        float* T = smemf + wv * 32 * TLD;                     // wave-private: no workgroup barrier inside the epilogue
        const int piece = lane % (TWD / 4), prow = lane / (TWD / 4);
        const int cob = co0 + TWD * wm + 4 * piece;           // first of this lane's four output channels
        const sd_f4 bias4 = *(const sd_f4*)(sBias + TWD * wm + 4 * piece);             // staged by the prologue: no wait on vector memory
        __syncthreads();                                      // every wave's last fragment reads are done: the staging buffers are free
        // The shortcut reads of BOTH half tiles are requested up front and waited for once; no load from global memory sits between two of the
        // tile's stores (stores count in vmcnt: a load behind a store waits for that store to be acknowledged).  `inside` as below.
        auto tail = [&](const bool res, const bool inside) {
            sd_f4 rr[2][32 / PPI];
            if (res) {
#pragma unroll
                for (int n = 0; n < 2; n++)
#pragma unroll
                    for (int it = 0; it < 32 / PPI; it++) {
                        const int p = pix0 + 64 * wn + 32 * n + PPI * it + prow;
                        rr[n][it] = sd_f4{0.f, 0.f, 0.f, 0.f};
                        if (inside || (p < npix && cob < A.cout)) rr[n][it] = *(const sd_f4*)(A.res + (size_t)p * A.resStride + cob);
                    }
                __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0)
            }
#pragma unroll
            for (int n = 0; n < 2; n++) {
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int g = 0; g < 4; g++)
                        *(sd_f4*)(T + r32 * TLD + 32 * m + 8 * g + 4 * h) = sd_f4{acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]};
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int pb = pix0 + 64 * wn + 32 * n;
#pragma unroll
                for (int it = 0; it < 32 / PPI; it++) {
                    const int pl = PPI * it + prow, p = pb + pl;
                    if (!inside && (p >= npix || cob >= A.cout)) continue;
                    const sd_f4 a = *(const sd_f4*)(T + pl * TLD + 4 * piece);
                    const sd_f4 v = sd_f32_tail(a, bias4, slope, rr[n][it], res);
                    float* dst = A.out + (size_t)p * A.outStride + cob;
                    if (inside || cob + 3 < A.cout) *(sd_f4*)dst = v;
                    else for (int e = 0; e < 4 && cob + e < A.cout; e++) dst[e] = v[e];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        };
        const bool inside = pix0 + BN <= npix && co0 + BM <= A.cout;
        if (A.res) { if (inside) tail(true, true); else tail(true, false); }
        else { if (inside) tail(false, true); else tail(false, false); }
    } else {
        // ---- epilogue: D column = pixel (lane & 31), rows = filters (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  All shortcut reads are
        // requested before the first one is used (one memory round trip, not one per 16-byte piece).
        // Then ONE wait on vector memory (none without a shortcut) and the wave's 16 stores back to back: stores count in vmcnt like loads, so
        // anything read from global memory between two stores -- the bias was, per piece -- waits for the store before it to be acknowledged:
        // 16 dependent round trips per wave and tile.  The bias comes from LDS (sBias, staged by the prologue).  `inside` (uniform per
        // workgroup): the tile lies wholly inside the pixels and the filters and needs no predicate per piece; edge tiles and the 255-filter heads
        // take the predicated form.  Both flags are literals at the call sites.
        // What it is aimed at: per layer, rate = A s / (s + c) with s the layer's K steps and A = 145 TFLOP/s -- every workgroup spends c = 5 - 8
        // K steps outside its K loop, whatever the layer (tools/conv_f32_fixed_cost.py).  Measured at batch 128, parent -> this epilogue, one box:
        // c 5.1 -> 4.4 (1 x 1 256 -> 128), 7.7 -> 6.4 (1 x 1 512 -> 256), 7.0 -> 6.2 (3 x 3 cin 128), 9.5 -> 8.6 (3 x 3 cin 256); the 1 x 1 layers - 3 %,
        // the 69 layers of this tile 107.8 -> 106.8 ms; headline 1063.1 -> 1076.2 frames/s (+ 1.2 %, four alternating runs each, parent spread 0.2 %:
        // profiles/conv_f32_epilogue_bench.json, _layers.txt, _isa.txt).  The results are bit for bit the parent's (tests/test_gpu_conv_f32_epilogue.py).
        // All eight bias pieces of a lane read up front instead of one per piece: 5 VGPRs spilled (168 + scratch) -- not kept.
        auto tail = [&](const bool res, const bool inside) {
            sd_f4 rr[2][MT][4];
            if (res) {
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    const int p = pix0 + 64 * wn + 32 * n + r32;
#pragma unroll
                    for (int m = 0; m < MT; m++)
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const int co = co0 + 32 * MT * wm + 32 * m + 8 * g + 4 * h;
                            rr[n][m][g] = sd_f4{0.f, 0.f, 0.f, 0.f};
                            if (inside || (p < npix && co < A.cout)) rr[n][m][g] = *(const sd_f4*)(A.res + (size_t)p * A.resStride + co);
                        }
                }
                __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0): every shortcut piece is here before the first store is issued
            }
#pragma unroll
            for (int n = 0; n < 2; n++) {
                const int p = pix0 + 64 * wn + 32 * n + r32;
                if (!inside && p >= npix) continue;
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int cl = 32 * MT * wm + 32 * m + 8 * g + 4 * h, co = co0 + cl;
                        if (!inside && co >= A.cout) continue;
                        const sd_f4 b4 = *(const sd_f4*)(sBias + cl);      // per piece: eight more live pieces beside rr and acc spill
                        const sd_f4 v = sd_f32_tail(sd_f4{acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]}, b4, slope, rr[n][m][g], res);
                        float* dst = A.out + (size_t)p * A.outStride + co;
                        if (inside || co + 3 < A.cout) *(sd_f4*)dst = v;
                        else for (int e = 0; e < 4 && co + e < A.cout; e++) dst[e] = v[e];
                    }
            }
        };
        const bool inside = pix0 + BN <= npix && co0 + BM <= A.cout;
        if (A.res) { if (inside) tail(true, true); else tail(true, false); }
        else { if (inside) tail(false, true); else tail(false, false); }
    }
}
#define SD_F32_LDS(BK, WM, MT, NW) (2 * (32 * (MT) * (WM) + 64 * ((NW) / (WM))) * ((BK) + 4) * 4 + 32 * (MT) * (WM) * 4)      // two stages + the tile's bias

// blobFromImage as k_blob_from_image, NHWC f32 with 4 channels (R, G, B after swapRB, then a zero)
__global__ void __launch_bounds__(256) k_blob_from_image_f32(const uint8_t* __restrict__ src, int sw, int sh, size_t sstride, size_t spitch,
                                                             const short4* __restrict__ ct, const short4* __restrict__ rt,
                                                             float* __restrict__ dst, int dw, int dh, int swapRB)
{
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dw || y >= dh) return;
    const short4 ce = ct[x], re = rt[y];
    const int sx = ce.x, sx1 = min(sx + 1, sw - 1);
    const int r0 = min(max((int)re.x, 0), sh - 1), r1 = min(max((int)re.x + 1, 0), sh - 1);
    const uint8_t* S0 = src + (size_t)img * spitch + (size_t)r0 * sstride;
    const uint8_t* S1 = src + (size_t)img * spitch + (size_t)r1 * sstride;
    // the two source pixels of a row are six consecutive bytes: one unaligned dword + one unaligned halfword per row instead of six byte loads (the
    // kernel was bound by the issue of its twelve byte loads per output pixel, not by its 16-byte store); the last source column repeats itself
    // (sx1 == sx) and takes the byte path, which never reads past its pixel
    uint32_t a0, a1, b0, b1;                                    // bytes 0-3 and 4-5 of the pair, rows r0 / r1
    if (sx1 == sx + 1) {
        typedef uint32_t __attribute__((aligned(1))) u32u; typedef uint16_t __attribute__((aligned(1))) u16u;
        a0 = *(const u32u*)(S0 + 3 * sx); b0 = *(const u16u*)(S0 + 3 * sx + 4);
        a1 = *(const u32u*)(S1 + 3 * sx); b1 = *(const u16u*)(S1 + 3 * sx + 4);
    } else {
        a0 = (uint32_t)S0[3 * sx] | ((uint32_t)S0[3 * sx + 1] << 8) | ((uint32_t)S0[3 * sx + 2] << 16) | ((uint32_t)S0[3 * sx1] << 24);
        b0 = (uint32_t)S0[3 * sx1 + 1] | ((uint32_t)S0[3 * sx1 + 2] << 8);
        a1 = (uint32_t)S1[3 * sx] | ((uint32_t)S1[3 * sx + 1] << 8) | ((uint32_t)S1[3 * sx + 2] << 16) | ((uint32_t)S1[3 * sx1] << 24);
        b1 = (uint32_t)S1[3 * sx1 + 1] | ((uint32_t)S1[3 * sx1 + 2] << 8);
    }
    const int p0[6] = {(int)(a0 & 255), (int)((a0 >> 8) & 255), (int)((a0 >> 16) & 255), (int)(a0 >> 24), (int)(b0 & 255), (int)((b0 >> 8) & 255)};
    const int p1[6] = {(int)(a1 & 255), (int)((a1 >> 8) & 255), (int)((a1 >> 16) & 255), (int)(a1 >> 24), (int)(b1 & 255), (int)((b1 >> 8) & 255)};
    float ch[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int h0 = p0[c] * ce.y + p0[3 + c] * ce.z;
        const int h1 = p1[c] * ce.y + p1[3 + c] * ce.z;
        const int v = ((((int)re.y * (h0 >> 4)) >> 16) + (((int)re.z * (h1 >> 4)) >> 16) + 2) >> 2;
        ch[c] = (float)(v & 255) * (float)(1 / 255.0);
    }
    float* o = dst + ((size_t)img * dh * dw + (size_t)y * dw + x) * 4;
    *(sd_f4*)o = sd_f4{swapRB ? ch[2] : ch[0], ch[1], swapRB ? ch[0] : ch[2], 0.f};
}


// [upsample] x 2 (nearest) of `a` (C1 channels at stride aStride, h x w) into channels [0, C1) of `out` (2h x 2w, Ct channels per pixel).  The second
// input of the [route] is not touched: in the f32-class modes its producer writes it in place (sd_yolo_create_prec).  One 16-byte piece per thread:
// a piece is read once per output pixel (four times in all, three of them from L2) and written once.
__global__ void __launch_bounds__(256) k_upsample_into_f32(const float* __restrict__ a, int C1, int aStride, int h, int w, float* __restrict__ out, int Ct, int N)
{
    const int q = C1 / 4, H2 = 2 * h, W2 = 2 * w;
    const size_t total = (size_t)N * H2 * W2 * q;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c4 = (int)(i % q);
        const size_t p = i / q;
        const int x = (int)(p % W2);
        const size_t r = p / W2;
        const int y = (int)(r % H2), n = (int)(r / H2);
        *(sd_f4*)(out + p * Ct + 4 * c4) = *(const sd_f4*)(a + (((size_t)n * h + (y >> 1)) * w + (x >> 1)) * aStride + 4 * c4);
    }
}
