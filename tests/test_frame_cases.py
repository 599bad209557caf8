"""CPU: the crafted sets of frame_cases.py hold the edges they claim, and the module's numpy references equal the oracle's."""
import importlib.util
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import frame_cases as fc
import stereo_cases as sc

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def CO():
    spec = importlib.util.spec_from_file_location("sd_cloud_oracle_cases", os.path.join(graft.ROOT, "oracle", "cloud_oracle.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


# ---- dense cloud
def test_records_mirror_the_header(pkg):
    fe = pkg.frontend
    assert fc.BOXES_DTYPE.itemsize == fe.FRAME_BOXES_BYTES and fc.CLOUD_POINT_DTYPE == fe.CLOUD_POINT_DTYPE and fc.MAXB == fe.MAXB
    assert (fc.GRID_COLS, fc.GRID_ROWS, fc.GRID_CELLS) == (fe.GRID_COLS, fe.GRID_ROWS, fe.GRID_CELLS)
    hdr = open(os.path.join(graft.ROOT, "include", "sd_frontend.h")).read()
    body = hdr[hdr.index("typedef struct sd_frame_boxes {"):hdr.index("} sd_frame_boxes;")]
    order = [body.index(n) for n in ("nb,", "n_all,", "n_static,", "n_dynamic;", "boxes[", "box_idx[", "box_status[", "kept_orig[", "box_start[", "pad_;")]
    assert order == sorted(order) and list(fc.BOXES_DTYPE.names) == ["nb", "n_all", "n_static", "n_dynamic", "boxes", "box_idx", "box_status", "kept_orig", "box_start", "pad_"]


def test_cloud_geometries_reach_the_three_layouts():
    shapes = {n: fc.cloud_shape(sc.GEOMS[n]) for n in fc.CLOUD_GEOMS}
    c, r, w, _ = shapes["752x240-8x1.2"]
    assert (c, w) == (251, 4) and c % 64 != 0                              # a ragged last word
    c, r, w, _ = shapes["1241x376-8x1.2"]
    assert w == 7 and w % 4 != 0                                           # the second pass of four waves has an idle one
    c, r, w, _ = shapes["1280x1008-5x2.0"]
    assert r == 336 > 256                                                  # the row-offset loop runs more than once per thread


def test_depth_window_values_lie_on_both_sides_of_both_bounds():
    v = np.array(fc.WINDOW_U16, np.uint16)
    for f in fc.FACTORS:
        d = v.astype(F32) * F32(f)
        low = d.astype(F64) < 0.01; high = d > F32(5.0)
        assert low.any() and (~low & ~high).any() and high.any()
        assert low[v == 0].all() and not low[v == 51].any() and not high[v == 5000].any() and high[v == 65535].all()
        # a value that is dropped only because the comparison is made in f64: d == 0.01f, which is below 0.01
        # (factor 1 / 5000 has one, the value 50; under 1 / 1000 the value 10 gives the f32 above 0.01f and is kept, 9 is dropped)
        on = d == F32(0.01)
        if f == fc.FACTORS[0]:
            assert on.any() and low[on].all() and not (d[on] < F32(0.01)).any(), "factor %r: no sample at 0.01f" % f
        else:
            assert low[v == 9].all() and not low[v == 10].any()
        # a value exactly on 5.0f is kept (`d > 5`), the next one is dropped
        on5 = d == F32(5.0)
        assert on5.any() and not high[on5].any() and high[np.nonzero(on5)[0] + 1].all(), "factor %r: no sample at 5.0f" % f
    assert (v.astype(F32) * F32(fc.FACTORS[0]))[v == 50] == F32(0.01)       # the case the issue names: 50 / 5000


@pytest.mark.parametrize("gname", fc.CLOUD_GEOMS)
def test_cloud_patterns_hold_their_edges(gname, CO):
    g = sc.GEOMS[gname]
    cols3, rows3, words, cap = fc.cloud_shape(g)
    cam = fc.cloud_camera(g)
    assert cam["cx"] != np.floor(cam["cx"]) and cam["cy"] != np.floor(cam["cy"])
    seen = {}
    for call in fc.cloud_calls(g):
        assert sorted(set(call["slots"])) != call["slots"] and len(set(call["slots"])) < len(call["slots"]) == 3     # out of order, one twice
        frames = fc.cloud_frames(g, call)
        assert len({f["Twc"].tobytes() for f in frames}) == 3 and len({f["color"].tobytes() for f in frames}) == 3
        for fr in frames:
            R = fr["Twc"][:3, :3]
            assert np.allclose(R @ R.T, np.eye(3)) and np.abs(R - np.eye(3)).min() > 1e-3 and np.abs(fr["Twc"][:3, 3]).min() > 0.01
        for fi, (kind, fr) in enumerate(zip(call["images"], frames)):
            fc.check_domain_cloud(g, fr, call["factor"])
            mask = fr["mask"] if call["use_mask"] else None
            pts, masked, keep, skip, d = fc.np_cloud(fr["color"], fr["depth"], call["factor"], mask, fr["boxes"], fr["status"], cam, fr["Twc"], detail=True)
            ref, rmasked = fc.oracle_cloud(CO, fr, call["factor"], call["use_mask"], cam)
            assert masked == rmasked and pts.tobytes() == ref.tobytes(), "%s %s: the two statements differ" % (call["name"], kind)
            assert (pts["a"] == 255).all()
            seen[(call["name"], fi)] = (keep, skip, d, fr, masked)
            # off the sample grid the image holds the other decision: reading a neighbour instead would change the count
            off = fr["depth"][1::3, 1::3].astype(F32) * F32(call["factor"])
            if kind in ("all", "none"):
                assert ((off.astype(F64) < 0.01) | (off > 5)).all() == (kind == "all")
    keep, skip, d, fr, _ = seen[("window-f0", 0)]
    for v in fc.WINDOW_U16:
        assert (fr["depth"][::3, ::3] == v).any() and (fr["depth"][1::3, 2::3] == v).any()
    assert keep[d == F32(5.0)].all() and not keep[d == F32(0.01)].any() and (d == F32(0.01)).any() and (d == F32(5.0)).any()
    keep, skip, *_ = seen[("window-f0", 1)]
    assert keep.all() and keep.sum() == cap and not skip.any()             # the count equals the least cap_points the ABI accepts
    keep, *_ = seen[("patterns", 0)]
    assert not keep.any()
    keep, *_ = seen[("patterns", 1)]
    assert keep.sum() == 1 and keep[-1, -1]
    keep, *_ = seen[("window-f0", 2)]
    assert keep[0, 63] and not keep[0, 64] and keep[1, 64] and not keep[1, 63] and keep[2, 63] and keep[2, 64] and keep.sum(1).max() == 2
    assert not keep[:, :63].any() and not keep[:, 65:].any()               # lane 63 of word 0, lane 0 of word 1, nothing else
    keep, *_ = seen[("patterns", 2)]
    full = keep.all(1); empty = ~keep.any(1)
    assert (full | empty).all() and full[1] and empty[2] and full[3] and full[-1] and empty.sum() >= rows3 // 5 - 1
    # boxes: the decisions on the box edges, under the mask
    keep, skip, d, fr, masked = seen[("boxes-mask", 0)]
    assert set(fr["status"]) == {-1, 0, 1, 2}
    s = lambda m, n: bool(skip[m // 3, n // 3])
    assert s(30, 30) and s(57, 57) and not s(30, 60) and not s(60, 30) and not s(27, 30)        # x = 30, w = 30: sample 30 in, 60 out
    assert not s(93, 90) and s(93, 93) and s(93, 120) and not s(93, 123) and not s(90, 93) and s(120, 93)      # x = 90.5: 90 out, 93 in
    assert not s(33, 150) and not s(30, 501)                               # zero width, zero height
    assert s(150, 0) and s(150, 12) and not s(150, 15)                     # negative x
    W3, H3 = 3 * (cols3 - 1), 3 * (rows3 - 1)
    assert s(H3, W3) and g.W - 20 + 100 > g.W                              # a box reaching past the image
    assert not s(39, 39) and fr["mask"][39, 39] == 0                       # mask zero inside a dynamic box: kept
    assert keep[13, 13]
    assert not s(69, 240) and s(63, 231) and s(87, 255)                    # the overlap: zero mask kept, the rest masked once
    assert not s(33, 330) and not s(33, 420)                               # box_status 1 and -1
    assert not s(3, 3) and fr["mask"][3, 3] != 0                           # mask non-zero outside every box: kept
    assert set(np.unique(fr["mask"][::3, ::3][skip])) == {1, 255}          # both non-zero values mask
    assert s(33, 201) and d[11, 67] == 0 and not keep[11, 67]              # masked and out of the window: still in masked_num
    assert masked == skip.sum() > (skip & keep_window(d)).sum()
    inb = np.zeros(skip.shape, int)
    for (x, y, w, h), stt in zip(fr["boxes"], fr["status"]):
        if stt in (0, 2):
            mm, nn = np.meshgrid(np.arange(0, g.H, 3), np.arange(0, g.W, 3), indexing="ij")
            inb += (x <= nn) & (nn < x + w) & (y <= mm) & (mm < y + h)
    assert (inb >= 2).any() and skip[inb >= 2].any() and skip.max() == 1   # a sample in two dynamic boxes counts once
    # slot 0 of the same call: 64 boxes, only the last dynamic
    _, s0, _, fr0, m0 = seen[("boxes-mask", 1)]
    assert len(fr0["status"]) == 64 and (fr0["status"][:63] != 0).all() and (fr0["status"][:63] != 2).all() and fr0["status"][63] == 2
    assert s0[50, 60] and not s0[35, 40] and m0 == s0.sum() > 0            # (150, 180) inside box 63; (105, 120) only inside the static ones
    # the same frames without a mask pointer: nothing masked although the dynamic boxes are there
    assert seen[("boxes-nomask", 0)][4] == 0 and not seen[("boxes-nomask", 0)][1].any()
    assert fc.box_set(g, "none")[0].shape == (0, 4)


def keep_window(d):
    return ~((d.astype(F64) < 0.01) | (d > F32(5.0)))


def test_padded_layout():
    img = np.arange(2 * 3 * 4, dtype=np.uint16).reshape(2, 3, 4) + 1
    p = fc.padded(img, 6, 20, 999, tail=5)
    assert len(p) == 45 and p[0:4].tolist() == [1, 2, 3, 4] and p[4] == 999 and p[6] == 5 and p[20] == 13 and p[18] == 999 and p[44] == 999


# ---- grid
@pytest.mark.parametrize("origin", fc.GRID_ORIGINS)
def test_grid_sets_hold_their_edges(origin, orc):
    cam = fc.grid_camera(origin)
    cap = fc.GEOM.cap
    assert F32(64) / (cam["mnMaxX"] - cam["mnMinX"]) == F32(0.125) == F32(48) / (cam["mnMaxY"] - cam["mnMinY"])
    for name, kp in fc.grid_sets(origin, cap):
        fc.check_domain_kp(kp, cam, cap)
        cell = fc.np_grid_cells(kp, cam)
        assert np.array_equal(cell, orc.grid_cells(kp, fc.cam10(cam))), name
        idx, start = fc.np_grid_index(cell)
        # the definition, member by member
        assert start[0] == 0 and start[-1] == (cell >= 0).sum() == len(idx) and len(start) == fc.GRID_CELLS + 1
        for c in np.unique(cell[cell >= 0]):
            assert idx[start[c]:start[c + 1]].tolist() == np.nonzero(cell == c)[0].tolist()
    sets = dict(fc.grid_sets(origin, cap))
    kp, pos = fc.grid_edges(origin)
    cell = fc.np_grid_cells(kp, cam)
    gx = (kp["x"] - cam["mnMinX"]) * F32(0.125); gy = (kp["y"] - cam["mnMinY"]) * F32(0.125)
    for h in fc.HALF_POS:                                                   # the exact halves are exact halves in f32, in x and in y
        assert (gx == F32(h)).any(), h
    for h in (-0.5, 0.5, 31.5, 46.5, 47.5):
        assert (gy == F32(h)).any(), h
    px = np.where(cell >= 0, cell // 48, -1); py = np.where(cell >= 0, cell % 48, -1)
    at = lambda x, y: int(cell[np.nonzero((pos[:, 0] == x) & (pos[:, 1] == y))[0][0]])
    assert at(0.5, 5.0) == 1 * 48 + 5 and at(1.5, 5.0) == 2 * 48 + 5 and at(62.5, 5.0) == 63 * 48 + 5      # halves round away from zero
    assert at(-0.5, 5.0) == -1 and at(-0.4, 5.0) == 5 and at(63.5, 5.0) == -1 and at(64.0, 5.0) == -1 and at(63.4375, 5.0) == 63 * 48 + 5
    assert at(7.0, -0.5) == -1 and at(7.0, -0.4) == 7 * 48 and at(7.0, 47.5) == -1 and at(7.0, 46.5) == 7 * 48 + 47 and at(7.0, 48.0) == -1
    assert at(-0.0625, 5.0) == 5
    # a truncating round would disagree on these
    wrong = ((gx + F32(0.5)).astype(np.int32) != fc.c_roundf(gx)) | ((gy + F32(0.5)).astype(np.int32) != fc.c_roundf(gy))
    assert wrong.any()
    if origin == (0.0, 0.0):
        assert (gx == np.nextafter(F32(0.5), F32(0))).any() and (gx == np.nextafter(F32(63.5), F32(0))).any()
    assert (fc.np_grid_cells(sets["all_out"], cam) == -1).all() and len(sets["all_out"]) > 256
    assert (fc.np_grid_cells(sets["one_cell"], cam) == fc.HEAVY_CELL).all() and len(sets["one_cell"]) == 600
    assert (fc.np_grid_cells(sets["one_cell_cap"], cam) == 1535).all() and len(sets["one_cell_cap"]) == cap
    cell = fc.np_grid_cells(sets["heavy"], cam)
    n = np.bincount(cell, minlength=fc.GRID_CELLS)
    assert n[fc.HEAVY_CELL] > 256 and all(n[c] == 1 for c in fc.SEAM_CELLS) and n[1] == 0 and n.sum() == 300 + len(fc.SEAM_CELLS)
    assert (np.diff(cell) < 0).any() and cell[3] == 3071                  # index order is not cell order
    assert {len(sets["count%d" % k]) for k in fc.GRID_COUNTS} == set(fc.GRID_COUNTS) and len(sets["count%d" % cap]) == cap
    for k in (255, 256, 257, cap):
        c = fc.np_grid_cells(sets["count%d" % k], cam)
        assert (c < 0).any() and (c >= 0).any() and (np.diff(c[c >= 0]) < 0).any()
    # under the distortion the same sets stay inside the domain
    for name, kp in fc.grid_sets(origin, cap):
        fc.check_domain_kp(kp, cam, cap, (fc.GRID_K4, fc.GRID_D5))


# ---- undistortion and bounds
def test_undistortion_sets(orc):
    pts, names = fc.undistort_points()
    assert len(pts) >= max(fc.UN_COUNTS) and set(fc.UN_COUNTS) == {0, 1, 255, 256, 257}
    P = dict(zip(names, pts))
    assert tuple(P["corner11"]) == (640, 480) and tuple(P["left"]) == (-50, 240) and tuple(P["bottom"]) == (320, 530)
    assert P["principal"][0] == fc.TUM1_K4[2] and P["principal"][1] == fc.TUM1_K4[3]
    sets = dict(fc.coefficient_sets())
    for i, n in enumerate(("k1", "k2", "p1", "p2", "k3")):
        assert np.count_nonzero(sets[n]) == 1 and sets[n][i] != 0
    assert sets["k1_zero"].tolist() == F32([0, .1, .01, .01, .1]).tolist()
    for name, d5 in sets.items():
        out = fc.check_domain_undistort(pts, fc.TUM1_K4, d5)
        assert np.array_equal(fc.bits(out), fc.bits(orc.undistort_points(pts, fc.TUM1_K4, d5))), name
        four = fc.np_undistort(pts, fc.TUM1_K4, d5, iters=4)
        assert (fc.bits(four) != fc.bits(out)).any(), "%s: a fifth iteration must show" % name
        assert np.array_equal(fc.bits(out[names.index("principal")]), fc.bits(pts[names.index("principal")]))      # the fixed point
        b = fc.np_image_bounds(fc.UN_W, fc.UN_H, fc.TUM1_K4, d5)
        assert np.array_equal(fc.bits(b), fc.bits(orc.image_bounds(fc.UN_W, fc.UN_H, fc.TUM1_K4, d5))), name
        if d5[0] == 0:
            assert b.tolist() == [0, 640, 0, 480] and np.abs(out - pts).max() > 0.5      # the points move, the key points and bounds must not
    assert np.abs(fc.np_undistort(pts, fc.TUM1_K4, sets["tum1"]) - pts).max() > 5


# ---- UnprojectStereo
def test_unproject_sets(orc):
    cam = fc.grid_camera((0.0, 0.0))
    for n, seed in ((0, 0), (1, 1), (257, 2), (fc.GEOM.cap, 3)):
        kp, d = fc.unproject_frame(n, seed, cam)
        fc.check_domain_depth(d)
        for k in range(2):
            T = fc.pose(k).astype(F32)
            xw, ok = fc.np_unproject(kp, d, cam, T)
            rxw, rok = orc.unproject(kp, d, fc.cam10(cam), T)
            assert np.array_equal(fc.bits(xw), fc.bits(rxw)) and np.array_equal(ok, rok)
        if n >= 24:
            e = fc.EDGE_DEPTHS
            assert np.array_equal(fc.bits(d[:8]), fc.bits(e)) and np.isnan(e[3]) and np.signbit(e[2]) and e[2] == 0
            tiny = np.finfo(F32).tiny
            assert 0 < e[5] < tiny < e[4]                                  # 1e-38 is itself subnormal
            assert (kp["x"][:8] == cam["cx"]).all() and (kp["y"][:8] == cam["cy"]).all()
            assert ok[:8].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
            x = (kp["x"] - cam["cx"]) * d * (F32(1) / cam["fx"])
            with np.errstate(invalid="ignore"):
                assert ((np.abs(x) > 0) & (np.abs(x) < tiny)).any()        # a subnormal product: a flushing build would show
    assert not np.isinf(fc.EDGE_DEPTHS).any()
    with pytest.raises(AssertionError):
        fc.check_domain_depth(np.array([np.inf], F32))


# ---- cvtColor, depth, Hamming
def test_cvt_gray_statements_agree(orc):
    for channels in (3, 4):
        img = fc.all_triples(channels)
        assert len(np.unique(img[..., :3].reshape(-1, 3).astype(np.uint32) @ np.array([1, 256, 65536], np.uint32))) == 1 << 24
        for rgb in (1, 0):
            if channels == 4 and rgb == 0:
                continue
            assert np.array_equal(fc.np_cvt_gray(img, rgb), orc.cvt_gray(img, rgb))
    a = fc.all_triples(4, 0); b = fc.all_triples(4, 1)
    assert (a[..., 3] != b[..., 3]).any() and np.array_equal(a[..., :3], b[..., :3])
    assert {1, 3, 4, 5, 15, 16, 17, 31, 33, 1023, 1024, 1025} == set(fc.CVT_WIDTHS) and {1, 3, 4, 5} == set(fc.CVT_HEIGHTS)
    im = fc.cvt_images(17, 3, 3)
    assert (fc.np_cvt_gray(im, 1) != fc.np_cvt_gray(im, 0)).any()


def test_depth_and_hamming_sets(orc):
    v = fc.all_u16()
    assert len(np.unique(v)) == 65536
    for f in fc.DEPTH_FACTORS:
        assert np.array_equal(fc.bits(fc.np_depth_to_f32(v, f)), fc.bits(orc.depth_to_f32(v, f)))
    assert len(fc.DEPTH_FACTORS) == 4 and fc.DEPTH_FACTORS[3] == 1.0
    seen = set()
    sizes = set()
    for a, b, planted in fc.hamming_sets():
        D = fc.np_hamming(a, b)
        j = np.arange(len(b))
        assert np.array_equal(D[j % len(a), j], planted)
        assert D[0, 0] == orc.descriptor_distance(a[0], b[0])
        seen.update(int(x) for x in planted); sizes.add((len(a), len(b)))
    assert seen == set(range(257)) and sizes == {(x, y) for x in fc.HAMMING_SIZES for y in fc.HAMMING_SIZES}
