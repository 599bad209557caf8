"""The detector's dispatch, pinned on the CPU: csrc/sd_yolo_plan.h (pure host code, compiled here with g++ alone) must plan, for every
convolution of yolov3.cfg, the launch the hand-written dispatch it replaced issued -- kernel, grid, block, tilesX, tilesY, groupY, the
map width that sizes the limb kernels' LDS, the Winograd input transform's grid.  Every kernel that could serve a layer is inside the
parity tolerance (and in f16 mode bit-identical), so a layer that falls to a slower kernel passes every numerical test: this one fails.
The expected records (tests/golden/yolo_launch_plan.json) were printed by the dispatch code of the commit named in the file (how: the
file's "what"); they are never regenerated from the code under test."""
import json
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = {"f16": 0, "f32": 1, "f32w": 2, "f32x3": 3}
# 640 x 480: n = 1 and 2 straddle the f16 mode's npix >= 512 rule on the 20 x 15 maps, 128 and 256 are the measured batch sizes;
# 352 x 224 at n = 3: the odd maps of test_f32_modes_odd_feature_maps_and_batch
CASES = [(p, 640, 480, n) for p in PRECS for n in (1, 2, 128, 256)] + [(p, 352, 224, 3) for p in PRECS]
CLS_WINO = 3            # SdYoloClass


def _key(p, w, h, n):
    return "%s %dx%d n=%d" % (p, w, h, n)


@pytest.fixture(scope="module")
def planned():
    """{case key: [(record string as in the golden file, filters, size, cinPad, class)]} from one run of tests/cpp/yolo_plan_dump.cpp."""
    d = tempfile.mkdtemp(prefix="yolo_plan_")
    exe = os.path.join(d, "yolo_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "slam-dynamic_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "yolo_plan_dump.cpp")])
    args = [str(v) for (p, w, h, n) in CASES for v in (PRECS[p], w, h, n)]
    out, cur = {}, None
    names = {v: k for k, v in PRECS.items()}
    for line in subprocess.check_output([exe] + args, text=True).splitlines():
        if line.startswith("case "):
            p, w, h, n = (int(v) for v in line.split()[1:])
            cur = out.setdefault(_key(names[p], w, h, n), [])
        else:
            layer, kernel, nums, shape = line.split("|")
            cur.append(("%s|%s|%s" % (layer, kernel, nums),) + tuple(int(v) for v in shape.split()))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "yolo_launch_plan.json")) as f:
        g = json.load(f)
    assert len(g["parent_commit"]) == 40
    return g["cases"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: _key(*c))
def test_launch_records_equal_the_replaced_dispatch(planned, golden, case):
    got, exp = [r[0] for r in planned[_key(*case)]], golden[_key(*case)]
    assert len(exp) == 75, "yolov3.cfg has 75 convolutions"
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g == e, "%s: planned %s, the replaced dispatch launched %s" % (_key(*case), g, e)


def _fields(rec):
    layer, kernel, nums = rec.split("|")
    gx, gy, block, tx, ty, g, width, pre = (int(v) for v in nums.split())
    return int(layer), kernel, dict(gridX=gx, gridY=gy, block=block, tilesX=tx, tilesY=ty, groupY=g, width=width, inputGrid=pre)


@pytest.mark.parametrize("n", [1, 2, 128, 256])
def test_f32_tiles_by_filter_count(planned, n):
    """Derived by hand from the layer list: the first layer on <8,1,1,8>; the one 32-filter layer after it (1 x 1) on <16,1,1,4>; the
    four 64-filter layers (two at 320 x 240, two 1 x 1 at 160 x 120) on <16,1,2,4>; the other 69 on <16,2,2,4>."""
    recs = planned[_key("f32", 640, 480, n)]
    count = {}
    for rec, filters, size, cin, cls in recs:
        layer, kernel, f = _fields(rec)
        want = ("k_conv_f32<8, 1, 1, 8>" if layer == 0 else "k_conv_f32<16, 1, 1, 4>" if filters <= 32 else
                "k_conv_f32<16, 1, 2, 4>" if filters <= 64 else "k_conv_f32<16, 2, 2, 4>")
        assert kernel == want, (layer, filters, kernel)
        count[kernel] = count.get(kernel, 0) + 1
    assert count == {"k_conv_f32<8, 1, 1, 8>": 1, "k_conv_f32<16, 1, 1, 4>": 1, "k_conv_f32<16, 1, 2, 4>": 4, "k_conv_f32<16, 2, 2, 4>": 69}
    assert [size for rec, filters, size, cin, cls in recs if 0 < _fields(rec)[0] and filters <= 32] == [1]


@pytest.mark.parametrize("n", [1, 2, 128, 256])
def test_f32w_and_f32x3_layer_counts(planned, n):
    wino = [r for r in planned[_key("f32w", 640, 480, n)] if r[4] == CLS_WINO]
    assert len(wino) == 31 and all(_fields(r[0])[1] == "k_wino_gemm_f32<16, 2>" and _fields(r[0])[2]["inputGrid"] > 0 for r in wino)
    x3 = [_fields(r[0]) for r in planned[_key("f32x3", 640, 480, n)]]
    b3c = [f for _, k, f in x3 if k.startswith("k_conv3x3_b3c<")]
    b3f = [f for _, k, f in x3 if k.startswith("k_conv3x3_b3<")]
    assert len(b3c) == 29 and all(f["width"] in (80, 40, 20) and f["block"] == 512 for f in b3c)
    assert len(b3f) == 2 and all(f["width"] == 160 for f in b3f)
    # k_conv3x3_b3c is persistent: at most one workgroup per CU (256), a multiple of the 8 XCDs
    assert all(f["gridX"] <= 256 and f["gridX"] % 8 == 0 for f in b3c)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "f16"], ids=lambda c: _key(*c))
def test_group_y_divides_tiles_y_within_the_l2_share(planned, case):
    """groupY filter tiles are walked back to back on a pixel tile: it divides tilesY, and a group of more than one tile keeps its weights
    (bm filters x K floats; the limb kernels hold 3 bf16 = 1.5 floats per weight) at or below 2.5 MB.  The Winograd GEMM walks ALL filter
    tiles on a block tile by design (V, not the weights, is its big operand)."""
    bm_of = {"k_conv_f32<8, 1, 1, 8>": 32, "k_conv_f32<16, 1, 1, 4>": 32, "k_conv_f32<16, 1, 2, 4>": 64, "k_conv_f32<16, 2, 2, 4>": 128,
             "k_conv_b3<1>": 64, "k_conv_b3<2>": 128, "k_conv3x3_b3c<5>": 64, "k_conv3x3_b3c<6>": 64}
    for rec, filters, size, cin, cls in planned[_key(*case)]:
        layer, kernel, f = _fields(rec)
        assert f["tilesY"] >= 1 and f["groupY"] >= 1 and f["tilesY"] % f["groupY"] == 0, rec
        if cls == CLS_WINO:
            assert f["groupY"] == f["tilesY"], rec
            continue
        bm = bm_of.get(kernel, 128)                      # k_conv3x3_b3<NP, 2, 2>: 128
        limb = kernel.startswith(("k_conv_b3", "k_conv3x3_b3"))
        kdim = (8 if layer == 0 else cin) * size * size * (3 if limb else 2) // 2
        assert f["tilesY"] == (filters + bm - 1) // bm, rec
        if f["groupY"] > 1:
            assert f["groupY"] * bm * kdim * 4 <= 2560 * 1024, rec
        # the 1-D grid: pixel tiles rounded up to the 8 XCDs, times the filter tiles (k_conv3x3_b3c: persistent, checked above)
        if not kernel.startswith("k_conv3x3_b3c"):
            assert f["gridX"] == (f["tilesX"] + 7) // 8 * 8 * f["tilesY"] and f["gridY"] == 1, rec


def test_f16_small_maps_change_kernel_between_one_and_two_images(planned):
    """The 20 x 15 maps (layers 62 - 81): 300 pixels at n = 1 are below the 512-pixel tiles of the LDS-DMA kernels, so the 3 x 3 stride-1
    layers run k_conv3x3_flat and the others k_conv_mfma<64>; 600 pixels at n = 2 reach them: k_conv3x3_glds<80>, k_conv_glds<4, 1> for the
    1 x 1 layers and <4, 3> for the stride-2 layer 62 (2 pixel tiles x at most 8 filter tiles stay below the 256 tiles of the 8-wave form)."""
    def rows(n):
        return {_fields(r[0])[0]: (_fields(r[0])[1], r[2]) for r in planned[_key("f16", 640, 480, n)]}
    r1, r2 = rows(1), rows(2)
    small = [i for i in r1 if 62 <= i <= 81]
    assert len(small) == 16
    for i in small:
        size = r1[i][1]
        assert r1[i][0] == ("k_conv3x3_flat" if size == 3 and i != 62 else "k_conv_mfma<64>"), i
        assert r2[i][0] == ("k_conv_glds<4, 3>" if i == 62 else "k_conv3x3_glds<80>" if size == 3 else "k_conv_glds<4, 1>"), i
    assert r1[0][0] == r2[0][0] == "k_conv_first"
