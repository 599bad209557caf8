"""GPU parity of Frame::ComputeStereoMatches / ComputeStereoFromRGBD against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_stereo_matches_oracle(gpu, fe, orc, synth):
    cfg = synth.KITTI_STEREO
    frames = [synth.stereo_frame(seq=2, t=t) for t in range(3)]
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], 2 * len(frames))
    b.extract_host(np.stack([im for (l, r, _) in frames for im in (l, r)]))
    b.stereo_match(len(frames), cfg["bf"], cfg["fx"])
    for f, (l, r, _) in enumerate(frames):
        oL = orc.Extractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
        oR = orc.Extractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
        kL, dL = oL(l); kR, dR = oR(r)
        our, odep, osad, nm = orc.stereo_matches(oL, oR, kL, dL, kR, dR, cfg["bf"], cfg["fx"])
        ur, dep, sad = b.download_stereo(f)
        n = len(kL)
        assert nm > 100, "synthetic pair should produce stereo matches"
        assert np.array_equal(sad[:n], osad), "SAD distances, frame %d" % f
        assert np.array_equal(ur[:n].view(np.uint32), our.view(np.uint32)), "mvuRight, frame %d" % f
        assert np.array_equal(dep[:n].view(np.uint32), odep.view(np.uint32)), "mvDepth, frame %d" % f
    b.close()


def test_rgbd_depth_lookup_matches_oracle(gpu, fe, orc, synth):
    import torch
    cfg = synth.KITTI03_RGBD
    rgb, depth, _ = synth.rgbd_frame(seq=3, t=0)
    gray = orc.cvt_gray(rgb, 1)
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], 1)
    b.extract_host(gray[None])
    factor = np.float32(1.0) / np.float32(cfg["depth_map_factor"])
    d_dev = torch.from_numpy(depth.astype(np.int16)).cuda()
    b.rgbd_from_u16(d_dev.data_ptr(), cfg["width"], cfg["width"] * cfg["height"], 1, float(factor), cfg["bf"])
    ur, dep = b.download_rgbd(0)
    o = orc.Extractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    kp, _ = o(gray)
    our, odep = orc.stereo_from_rgbd(kp, orc.depth_to_f32(depth, float(factor)), cfg["bf"])
    n = len(kp)
    assert (odep > 0).sum() > 100
    assert np.array_equal(ur[:n].view(np.uint32), our.view(np.uint32))
    assert np.array_equal(dep[:n].view(np.uint32), odep.view(np.uint32))
    b.close()


def test_stereo_dense_band_takes_the_multi_pass_branches(gpu, fe, orc, synth):
    """All texture of a 752 x 160 pair sits in a 36-row band and the extractor is asked for 4000 features: a 16-row chunk of k_stereo_match then
    holds far more than SD_SR_LEFT (128) left key points and its row band more than SD_SR_CAND (256) right candidates, so the `lb` / `cb` pass
    loops (csrc/k_frame.h) run several times and `s_best` carries (distance, iR) across candidate passes -- the branches the KITTI / TUM
    geometries never reach.  Bit-exact against the oracle's Frame::ComputeStereoMatches (/root/reference/src/Frame.cc:874-1048)."""
    cfg = synth.KITTI_STEREO
    W, H = 752, 160
    rng = np.random.Generator(np.random.PCG64(20260104))
    left = np.full((H, W + 16), 128, np.uint8)
    for y in range(62, 98, 3):                          # 3 x 3 blocks of random intensity: corners everywhere in the band
        for x in range(0, W + 16, 3):
            left[y:y + 3, x:x + 3] = rng.integers(20, 236)
    right = np.ascontiguousarray(left[:, 9:9 + W])      # disparity 9 px
    left = np.ascontiguousarray(left[:, :W])
    NL = 5                                              # 160 rows: the sixth level would have no FAST cell left (spec Q8: unsupported geometry)
    ex = fe.ORBextractor(4000, cfg["scale_factor"], NL, cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, W, H, 2)
    try:
        b.extract_host(np.stack([left, right]))
        b.stereo_match(1, cfg["bf"], cfg["fx"])
        oL = orc.Extractor(4000, cfg["scale_factor"], NL, cfg["ini_th_fast"], cfg["min_th_fast"])
        oR = orc.Extractor(4000, cfg["scale_factor"], NL, cfg["ini_th_fast"], cfg["min_th_fast"])
        kL, dL = oL(left); kR, dR = oR(right)
        kpg, descg, _ = b.download(0)
        assert kpg.tobytes() == kL.tobytes() and np.array_equal(descg, dL), "left extraction"
        rows = np.floor(kL["y"]).astype(int)
        chunk = np.bincount(rows // 16, minlength=H // 16 + 1)
        assert chunk.max() > 2 * 128, "a 16-row chunk must hold several passes of left key points (has %d)" % chunk.max()
        rrows = np.floor(kR["y"]).astype(int)
        c = int(np.argmax(chunk))
        band = int(((rrows >= 16 * c - 9) & (rrows <= 16 * c + 24)).sum())
        assert band > 2 * 256, "the chunk's row band must hold several passes of right candidates (has %d)" % band
        our, odep, osad, nm = orc.stereo_matches(oL, oR, kL, dL, kR, dR, cfg["bf"], cfg["fx"])
        ur, dep, sad = b.download_stereo(0)
        n = len(kL)
        assert nm > 300, "the shifted pair must match (%d)" % nm
        assert np.array_equal(sad[:n], osad), "SAD distances"
        assert np.array_equal(ur[:n].view(np.uint32), our.view(np.uint32)), "mvuRight"
        assert np.array_equal(dep[:n].view(np.uint32), odep.view(np.uint32)), "mvDepth"
    finally:
        b.close()


# ---- crafted key points (tests/stereo_cases.py): the images only supply the pyramids, key points and descriptors are written over the
# extraction results.  tests/test_oracle_stereo.py pins which branch of Frame::ComputeStereoMatches every case reaches; here the device
# output of the same arrays must be the oracle's bytes.  All arithmetic involved is integer or single correctly rounded f32 operations.

import stereo_cases as sc  # noqa: E402


def _pyramid_check(orc):
    """The downloaded padded planes against the oracle extractor's, so that a window mismatch is not blamed on the matcher."""
    def check(f, c, b):
        for slot, e in zip((2 * f, 2 * f + 1), sc.oracle_extractors(orc, c)):
            for l in range(c["geom"].n_levels):
                assert np.array_equal(b.pyramid(slot, l), e.pyramid(l)), "%s: pyramid level %d of slot %d" % (c["name"], l, slot)
    return check


def _assert_cases(orc, ws, cases, what, check_pyramids=True):
    got = sc.run_cases(ws, cases, _pyramid_check(orc) if check_pyramids else None)
    res = [sc.oracle(orc, c) for c in cases]
    bad = ["%s [slot %d of %d]: %s" % (c["name"], f, len(cases), "; ".join(sc.compare(g_, o)))
           for f, (c, g_, o) in enumerate(zip(cases, got, res)) if sc.compare(g_, o)]
    print("%s: %d cases, %d left key points compared, outcomes %s, %d cases differ"
          % (what, len(cases), sum(len(c["kL"]) for c in cases), dict(zip(orc.ST_NAMES, sc.histogram(res).tolist())), len(bad)))
    assert not bad, "\n".join(bad)
    return got


@pytest.mark.parametrize("name", list(sc.GEOMS))
def test_crafted_cases_match_oracle(gpu, fe, orc, name):
    """Every case kind of stereo_cases.suite at one geometry, all cases in one launch."""
    g = sc.GEOMS[name]
    cases = sc.suite(g)
    ws = sc.Workspace(fe, g, len(cases))
    try:
        assert ws.cap == g.cap, "kp_capacity %d, the generators assume %d" % (ws.cap, g.cap)
        _assert_cases(orc, ws, cases, name)
    finally:
        ws.close()


def test_crafted_cases_do_not_depend_on_slot_or_neighbours(gpu, fe, orc):
    """1, 7, 8, 9, 17 frames per launch (the XCD-ordered grid is padded to a multiple of 8 frames): the same cases in different slots,
    with empty frames (0 left or 0 right key points) between full ones."""
    g = sc.GEOMS["752x240-8x1.2"]
    pool = [sc.shifted(g, 9), sc.counts(g, 0, 50), sc.hamming_ties(g), sc.counts(g, 50, 0), sc.window_edges(g), sc.counts(g, 0, 0),
            sc.zero_disparity(g), sc.exact_copy(g, 9), sc.left_passes(g), sc.hamming_passes(g, False)]
    ws = sc.Workspace(fe, g, 17)
    seen = {}
    try:
        for F in (1, 7, 8, 9, 17):
            cases = [pool[(k + F) % len(pool)] for k in range(F)]
            got = _assert_cases(orc, ws, cases, "%d frames per launch" % F, check_pyramids=F in (1, 17))
            for c, r in zip(cases, got):
                b = b"".join(a.tobytes() for a in r)
                assert seen.setdefault(c["name"], b) == b, "%s changed with its slot" % c["name"]
        assert len(seen) == len(pool)
    finally:
        ws.close()


def test_small_launch_after_a_full_one_on_the_same_workspace(gpu, fe, orc):
    """kp_capacity key points on both sides, then one key point, then the first again: the row tables and the result arrays are reused."""
    g = sc.GEOMS["1241x376-8x1.2"]
    ws = sc.Workspace(fe, g, 2)
    try:
        full, one = sc.counts(g, ws.cap, ws.cap), sc.counts(g, 1, 1)
        a = _assert_cases(orc, ws, [full, full], "capacity launch")
        _assert_cases(orc, ws, [one], "one key point after it", check_pyramids=False)
        _assert_cases(orc, ws, [one, sc.counts(g, 0, 0)], "one key point and an empty frame", check_pyramids=False)
        b = _assert_cases(orc, ws, [full, full], "capacity launch again", check_pyramids=False)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0] + a[1], b[0] + b[1]))
    finally:
        ws.close()


def test_band_larger_than_the_staged_row_slice_is_refused(gpu, fe, orc):
    """12 levels at 1.31: bandR = ceil(2 * 1.31^11) + 2 >= 41 and 16 + 2 * bandR + 2 > SD_SR_RS = 96.  The call returns SD_ERR_UNSUPPORTED
    with its message, and a valid call on another workspace afterwards is correct."""
    g = sc.REFUSED
    rng = np.random.default_rng([sc.SEED, 77])
    c = sc.case(g, "refused", sc.images(g, "shift", 9), *sc.pairs(g, rng, 40, 9))
    ws = sc.Workspace(fe, g, 1)
    try:
        with pytest.raises(fe.SdError) as e:
            sc.run_cases(ws, [c])
        assert e.value.code == fe.SD_ERR_UNSUPPORTED and "stereo row band larger than the staged row table" in str(e.value)
    finally:
        ws.close()
    g = sc.GEOMS["752x240-8x1.2"]
    ws = sc.Workspace(fe, g, 1)
    try:
        _assert_cases(orc, ws, [sc.shifted(g, 9)], "after the refusal")
    finally:
        ws.close()


# ---- ComputeStereoFromRGBD on crafted key points

def _rgbd_keypoints(g, rng, n):
    """The four corners, the same with fractions .999, and random positions."""
    W, H = g.W, g.H
    x = [0, W - 1, 0, W - 1, 0.999, W - 0.001, 0.999, W - 0.001]
    y = [0, 0, H - 1, H - 1, 0.999, 0.999, H - 0.001, H - 0.001]
    x = np.concatenate([x, rng.uniform(0, W - 0.01, n - 8)]); y = np.concatenate([y, rng.uniform(0, H - 0.01, n - 8)])
    return sc.kps(g, x, y, rng.integers(0, g.n_levels, n))


@pytest.mark.parametrize("distortion", [False, True])
def test_rgbd_crafted_key_points_all_entry_points(gpu, fe, orc, synth, distortion):
    """Crafted key points (corners, fractions .999) over depth maps with a row stride larger than the width and an image pitch larger
    than stride * H, three images; depth 0, negative, NaN, +inf, u16 0 and 65535 under key points; rgbd_from_u16, _f32 and
    _f32_scaled.  With a distortion set the lookup stays at mvKeys and the subtraction uses mvKeysUn.  Bit for bit."""
    import torch
    g = sc.GEOMS["752x240-8x1.2"]
    W, H, n_img, N = g.W, g.H, 3, 200
    stride, pitch = W + 5, (W + 5) * H + 17
    ws = sc.Workspace(fe, g, 2)
    b = ws.b
    try:
        if distortion:
            t = synth.TUM1
            b.set_distortion([t["fx"], t["fy"], t["cx"], t["cy"]], fe.distortion_of(t))
        b.extract_host(np.stack([sc.images(g, "shift", 9)[0]] * n_img)); b.sync()
        rng = np.random.default_rng([sc.SEED, 31, int(distortion)])
        keys = [_rgbd_keypoints(g, rng, N - 7 * i) for i in range(n_img)]
        for i, k in enumerate(keys):
            sc.check_domain(dict(name="rgbd", geom=g, left=sc.images(g, "shift", 9)[0], right=sc.images(g, "shift", 9)[0], kL=k,
                                 dL=np.zeros((len(k), 32), np.uint8), kR=k, dR=np.zeros((len(k), 32), np.uint8)), ws.cap)
            ws.kp[i, :k.nbytes] = torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).cuda()
        ws.count[:n_img] = torch.tensor([len(k) for k in keys], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b.undistort(list(range(n_img))); b.sync()
        keys_un = [b.download_keys_un(i) for i in range(n_img)]
        for k, ku in zip(keys, keys_un):
            assert len(ku) == len(k) and (np.array_equal(ku["x"], k["x"]) != distortion)
        # depth maps: random positive values, special ones under the key points in turn
        f32 = np.full(n_img * pitch, np.float32(-7), np.float32); u16 = np.full(n_img * pitch, 3, np.uint16)
        view = lambda a, i: a[i * pitch:i * pitch + stride * H].reshape(H, stride)
        special_f = np.float32([0.0, -1.5, np.nan, np.inf, 1e-30, 0.01, 80.0, -0.0])
        special_u = np.uint16([0, 65535, 1, 5000, 0, 65535, 2, 40000])
        for i, k in enumerate(keys):
            vf, vu = view(f32, i), view(u16, i)
            vf[:, :W] = rng.uniform(0.3, 60, (H, W)).astype(np.float32); vu[:, :W] = rng.integers(1, 65536, (H, W)).astype(np.uint16)
            r, c_ = k["y"].astype(np.int64), k["x"].astype(np.int64)
            sel = np.arange(0, len(k), 2)
            vf[r[sel], c_[sel]] = special_f[(sel // 2) % 8]; vu[r[sel], c_[sel]] = special_u[(sel // 2) % 8]
        d_f32 = torch.from_numpy(f32).cuda(); d_u16 = torch.from_numpy(u16.view(np.int16)).cuda()
        factor = np.float32(1.0) / np.float32(5000.0)
        runs = (("u16", lambda: b.rgbd_from_u16(d_u16.data_ptr(), stride, pitch, n_img, float(factor), g.bf),
                 lambda i: orc.depth_to_f32(np.ascontiguousarray(view(u16, i)[:, :W]), float(factor))),
                ("f32", lambda: b.rgbd_from_f32(d_f32.data_ptr(), stride, pitch, n_img, g.bf),
                 lambda i: np.ascontiguousarray(view(f32, i)[:, :W])),
                ("f32_scaled", lambda: b.rgbd_from_f32_scaled(d_f32.data_ptr(), stride, pitch, n_img, float(factor), g.bf),
                 lambda i: np.ascontiguousarray(view(f32, i)[:, :W]) * factor))
        for name, launch, depth_of in runs:
            launch()
            for i, (k, ku) in enumerate(zip(keys, keys_un)):
                ur, dep = b.download_rgbd(i)
                our, odep = orc.stereo_from_rgbd(k, depth_of(i), g.bf, ku if distortion else None)
                n = len(k)
                assert (odep > 0).sum() > 50 and (odep == -1).sum() > 10 and (np.isinf(odep).sum() > 0 or name == "u16")
                assert np.array_equal(ur[:n].view(np.uint32), our.view(np.uint32)), "%s: mvuRight, image %d" % (name, i)
                assert np.array_equal(dep[:n].view(np.uint32), odep.view(np.uint32)), "%s: mvDepth, image %d" % (name, i)
    finally:
        ws.close()
