"""GPU: frame preparation and the dense cloud on the crafted inputs of frame_cases.py, bit for bit against the oracle
(oracle/oracle.py, oracle/cloud_oracle.py).  Blank images, no tracker, no extraction of real content: the slots' device arrays are
written directly.  test_frame_cases.py shows on the CPU that the inputs hold the edges named here."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import frame_cases as fc
import stereo_cases as sc

pytestmark = pytest.mark.gpu
F32 = np.float32
Z5 = np.zeros(5, F32)


@pytest.fixture(scope="module")
def CO():
    spec = importlib.util.spec_from_file_location("sd_cloud_oracle_cases", os.path.join(graft.ROOT, "oracle", "cloud_oracle.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def wsof(gpu, fe):
    """One workspace per geometry, made on first use."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = fc.Workspace(fe, sc.GEOMS[name])
        return made[name]
    yield get
    for w in made.values():
        w.close()


def eq(a, b):
    a, b = fc.bits(a), fc.bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def undistorted(orc, kp, K4, d5):
    out = kp.copy()
    if len(kp) and d5[0] != 0:
        u = orc.undistort_points(np.stack([kp["x"], kp["y"]], 1), K4, d5)
        out["x"] = u[:, 0]; out["y"] = u[:, 1]
    return out


# ---- dense cloud
@pytest.mark.parametrize("gname", fc.CLOUD_GEOMS)
def test_dense_cloud(wsof, CO, gname):
    """Per geometry five launches of three frames (slots out of order, one twice; padded strides and pitches): both counters, every
    kept point's bytes, and the sentinel after the count.  cap_points is the least the ABI accepts, which the all-kept frame fills."""
    ws = wsof(gname)
    g, cam = ws.g, fc.cloud_camera(ws.g)
    cap = fc.cloud_shape(g)[3]
    filled = False
    for call in fc.cloud_calls(g):
        cnt, pts, frames, err = fc.run_cloud(ws, call)
        assert err is None, "%s: %s" % (call["name"], err)
        for f, fr in enumerate(frames):
            ref, masked = fc.oracle_cloud(CO, fr, call["factor"], call["use_mask"], cam)
            what = "%s %s frame %d (%s)" % (gname, call["name"], f, call["images"][f])
            assert (int(cnt[f, 0]), int(cnt[f, 1])) == (len(ref), masked), "%s: cloud size / masked_num %r vs %r" % (what, cnt[f], (len(ref), masked))
            got = pts[f, :len(ref)]
            if got.tobytes() != ref.tobytes():
                bad = np.nonzero((fc.bits(got).reshape(-1, 16) != fc.bits(ref).reshape(-1, 16)).any(1))[0]
                raise AssertionError("%s: %d of %d points differ, first %d: %r vs %r" % (what, len(bad), len(ref), bad[0], got[bad[0]], ref[bad[0]]))
            assert (ref["a"] == 255).all()
            assert (fc.bits(pts[f, len(ref):]) == fc.SENTINEL).all(), "%s: points written after the count" % what
            filled |= len(ref) == cap
    assert filled


def test_dense_cloud_on_a_fresh_workspace_and_two_streams(gpu, fe, CO):
    """Two calls on a fresh 752 x 240 workspace, each on a stream of its own: the first allocates the marks, both equal the oracle."""
    import torch
    ws = fc.Workspace(fe, sc.GEOMS[fc.CLOUD_GEOMS[0]])
    try:
        g, cam = ws.g, fc.cloud_camera(ws.g)
        assert (g.W, g.H) == (752, 240)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for call, st in zip(fc.cloud_calls(g)[:2], streams):
            cnt, pts, frames, err = fc.run_cloud(ws, call, stream=st.cuda_stream)
            assert err is None, "%s: %s" % (call["name"], err)
            for f, fr in enumerate(frames):
                ref, masked = fc.oracle_cloud(CO, fr, call["factor"], call["use_mask"], cam)
                assert (int(cnt[f, 0]), int(cnt[f, 1])) == (len(ref), masked) and pts[f, :len(ref)].tobytes() == ref.tobytes(), "%s frame %d" % (call["name"], f)
                assert (fc.bits(pts[f, len(ref):]) == fc.SENTINEL).all()
    finally:
        ws.close()


def test_dense_cloud_limits(wsof, fe):
    """n_frames = 0 does nothing; cap_points one below ceil(W / 3) * ceil(H / 3) is refused and nothing is written."""
    import torch
    ws = wsof(fc.CLOUD_GEOMS[0])
    g = ws.g
    cap = fc.cloud_shape(g)[3]
    call = fc.cloud_calls(g)[0]
    cnt, pts, _, err = fc.run_cloud(ws, call, cap_points=cap - 1)
    assert isinstance(err, fe.SdError) and err.code == fe.SD_ERR_CAPACITY
    assert (fc.bits(pts) == fc.SENTINEL).all() and (cnt == -7).all()
    buf = torch.full((64,), fc.SENTINEL, dtype=torch.uint8, device="cuda")
    ws.b.backproject_dense([], buf.data_ptr(), 3 * g.W, 3 * g.W * g.H, buf.data_ptr(), g.W, g.W * g.H, call["factor"], buf.data_ptr(), g.W, g.W * g.H,
                           fc.cloud_camera(g), np.zeros((0, 16)), buf.data_ptr(), cap, buf.data_ptr())
    ws.b.sync()
    assert (buf.cpu().numpy() == fc.SENTINEL).all()


# ---- grid
@pytest.mark.parametrize("dist", [False, True], ids=["plain", "distorted"])
@pytest.mark.parametrize("origin", fc.GRID_ORIGINS, ids=["origin0", "origin-13.5"])
def test_grid_cells_and_sorted_index(wsof, orc, origin, dist):
    """cellOf, sortedIdx[:total] and all 3073 cellStart entries of every crafted frame; two runs give the same bytes; the slots a call
    does not cover keep their index.  (The ABI's sd_batch_assign_grid covers slots 0 .. n - 1; a slot step exists only inside the tracker.)"""
    ws = wsof(fc.GEOM.name)
    b, cap = ws.b, ws.cap
    cam = fc.grid_camera(origin)
    d5 = fc.GRID_D5 if dist else Z5
    sets = fc.grid_sets(origin, cap)
    assert len(sets) > 2 * ws.n

    def expect(kp):
        fc.check_domain_kp(kp, cam, cap, (fc.GRID_K4, fc.GRID_D5) if dist else None)
        un = undistorted(orc, kp, fc.GRID_K4, d5)
        cell = orc.grid_cells(un, fc.cam10(cam))
        return (un, cell) + fc.np_grid_index(cell)

    def check(s, name, kp):
        un, cell, idx, start = expect(kp)
        what = "%s slot %d" % (name, s)
        assert b.download_keys_un(s).tobytes() == un.tobytes(), what
        got = b.download_grid(s)[:len(kp)]
        assert np.array_equal(got.astype(np.int32), cell), "%s: cellOf differs at %r" % (what, np.nonzero(got != cell)[0][:5])
        gi, gs = b.download_grid_index(s)
        assert len(gs) == fc.GRID_CELLS + 1 and np.array_equal(gs, start), "%s: cellStart differs at %r" % (what, np.nonzero(gs != start)[0][:5])
        assert np.array_equal(gi, idx), "%s: sortedIdx differs at %r of %d" % (what, np.nonzero(gi != idx)[0][:5] if len(gi) == len(idx) else len(gi), len(idx))
        return got.tobytes() + gi.tobytes() + gs.tobytes()

    b.set_distortion(fc.GRID_K4, d5)
    try:
        kept = None
        for i in range(0, len(sets), ws.n):
            grp = sets[i:i + ws.n]
            ws.set_kps({s: kp for s, (_, kp) in enumerate(grp)})
            b.undistort(list(range(len(grp))))
            if kept is not None and len(grp) > 2:
                b.assign_grid(2, cam)                                   # slots 2 and 3 hold new key points but are not in the call
                for s in (2, 3):
                    gi, gs = b.download_grid_index(s)
                    assert gi.tobytes() + gs.tobytes() == kept[s], "slot %d outside the call lost its index" % s
            runs = []
            for _ in range(2):
                b.assign_grid(len(grp), cam)
                runs.append([check(s, name, kp) for s, (name, kp) in enumerate(grp)])
            assert runs[0] == runs[1]
            if len(grp) == ws.n:
                kept = {s: b"".join(x.tobytes() for x in b.download_grid_index(s)) for s in (2, 3)}
    finally:
        b.set_distortion(fc.GRID_K4, Z5)


def test_grid_index_needs_an_assigned_grid(wsof, fe):
    ws = wsof(fc.GEOM.name)
    ws.b.extract_host(np.full((ws.n, ws.g.H, ws.g.W), 128, np.uint8))      # a fresh extraction: the slots hold no grid
    ws.b.sync()
    with pytest.raises(fe.SdError) as e:
        ws.b.download_grid_index(1)
    assert e.value.code == fe.SD_ERR_STATE
    ws.b.assign_grid(2, fc.grid_camera((0.0, 0.0)))
    idx, start = ws.b.download_grid_index(1)
    assert len(idx) == 0 and not start.any()
    with pytest.raises(fe.SdError) as e:
        ws.b.download_grid_index(2)
    assert e.value.code == fe.SD_ERR_STATE


# ---- UnprojectStereo
@pytest.mark.parametrize("dist", [False, True], ids=["plain", "distorted"])
@pytest.mark.parametrize("step", [1, 2])
def test_unproject(wsof, orc, step, dist):
    """Depths 0, -1, -0.0, NaN, 1e-30, 1e-38, 0.01, 80 against key points at (cx, cy) and elsewhere; counts cap, 0, 257, 1; a different
    pose per frame; the map-point table pre-filled, so that the entries past the count and the skipped slots show untouched."""
    ws = wsof(fc.GEOM.name)
    b, cap = ws.b, ws.cap
    cam = fc.grid_camera((0.0, 0.0))
    d5 = fc.GRID_D5 if dist else Z5
    counts = [cap, 0, 257, 1]
    frames = [fc.unproject_frame(n, s, cam) for s, n in enumerate(counts)]
    rng = np.random.default_rng(step)
    sent_xw = rng.normal(size=(ws.n, cap, 3)).astype(F32); sent_fl = rng.integers(2, 256, (ws.n, cap), dtype=np.uint8)
    n_frames = (ws.n + step - 1) // step
    Twc = np.stack([fc.pose(k + 1).astype(F32) for k in range(n_frames)])
    b.set_distortion(fc.GRID_K4, d5)
    try:
        for s, (kp, d) in enumerate(frames):
            fc.check_domain_kp(kp, cam, cap, (fc.GRID_K4, fc.GRID_D5) if dist else None); fc.check_domain_depth(d)
            b.set_mappoints(s, sent_xw[s], sent_fl[s])
        ws.set_kps({s: kp for s, (kp, _) in enumerate(frames)})
        ws.set_depth({s: d for s, (_, d) in enumerate(frames)})
        b.undistort(list(range(ws.n)))
        b.unproject(step, n_frames, cam, Twc)
        b.sync()
        xw = ws.xw.cpu().numpy(); fl = ws.flags.cpu().numpy()
    finally:
        b.set_distortion(fc.GRID_K4, Z5)
    for s, (kp, d) in enumerate(frames):
        exw, efl = sent_xw[s].copy(), sent_fl[s].copy()
        if s % step == 0:
            oxw, ok = orc.unproject(undistorted(orc, kp, fc.GRID_K4, d5), d, fc.cam10(cam), Twc[s // step])
            exw[:len(kp)] = oxw; efl[:len(kp)] = ok
            if len(kp) >= 8:
                assert ok[:8].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and np.abs(oxw[4:8]).max() > 0
        bad = np.nonzero((fc.bits(xw[s]) != fc.bits(exw)).any(1) | (fl[s] != efl))[0]
        assert len(bad) == 0, "slot %d (count %d): %d entries differ, first %d: %r %r vs %r %r (depth %r)" % (
            s, len(kp), len(bad), bad[0], xw[s, bad[0]], fl[s, bad[0]], exw[bad[0]], efl[bad[0]], d[bad[0]] if bad[0] < len(d) else None)


# ---- undistortion and bounds
def test_undistort_points_and_bounds(fe, gpu, orc):
    import torch
    pts, _ = fc.undistort_points()
    for name, d5 in fc.coefficient_sets():
        fc.check_domain_undistort(pts, fc.TUM1_K4, d5)
        for n in fc.UN_COUNTS:
            d_in = torch.from_numpy(pts).cuda(); d_out = torch.full((len(pts), 2), -77.25, dtype=torch.float32, device="cuda")
            fe.check(fe.lib().sd_undistort_points_device(C.c_void_p(d_in.data_ptr()), n, fe._p(fc.TUM1_K4), fe._p(d5), C.c_void_p(d_out.data_ptr()), None))
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert eq(got[:n], orc.undistort_points(pts[:n], fc.TUM1_K4, d5)), "%s n = %d" % (name, n)
            assert (got[n:] == -77.25).all()
        b = fe.image_bounds(fc.UN_W, fc.UN_H, fc.TUM1_K4, d5)
        assert eq(b, orc.image_bounds(fc.UN_W, fc.UN_H, fc.TUM1_K4, d5)), name
        if d5[0] == 0:
            assert b.tolist() == [0.0, float(fc.UN_W), 0.0, float(fc.UN_H)], name
        else:
            assert b.tolist() != [0.0, float(fc.UN_W), 0.0, float(fc.UN_H)], name


def test_undistort_keypoints_of_slots(wsof, fe, orc):
    """sd_batch_undistort_keypoints and sd_batch_undistort (static and dynamic key points) under every coefficient set: positions as the
    oracle's, every other field unchanged, identical records when k1 == 0, nothing written past the counts."""
    import torch
    ws = wsof(fc.GEOM.name)
    b, cap, g = ws.b, ws.cap, ws.g
    pts, _ = fc.undistort_points()
    counts = [257, 255, 256, 1]
    kps = [fc.frame_kps(pts[:n, 0], pts[:n, 1], s) for s, n in enumerate(counts)]
    kps0 = [fc.frame_kps(pts[:n, 0], pts[:n, 1], s) for s, n in enumerate([0, 300, 0, 2])]
    for k in kps + kps0:
        assert len(k) == 0 or len(set(map(bytes, fc.bits(k).reshape(len(k), -1)[:, 8:]))) > len(k) // 2      # the other fields differ
    nrec = fc.KP_DTYPE.itemsize
    for name, d5 in fc.coefficient_sets():
        for group in (kps, kps0):
            ws.set_kps(dict(enumerate(group)))
            d_un = torch.full((ws.n, cap, nrec), 0x6B, dtype=torch.uint8, device="cuda")
            fe.check(fe.lib().sd_batch_undistort_keypoints(b.h, ws.n, fe._p(fc.TUM1_K4), fe._p(d5), C.c_void_p(d_un.data_ptr()), None))
            b.sync()
            got = d_un.cpu().numpy()
            for s, kp in enumerate(group):
                exp = undistorted(orc, kp, fc.TUM1_K4, d5)
                assert got[s, :len(kp)].tobytes() == exp.tobytes(), "%s slot %d" % (name, s)
                assert (got[s, len(kp):] == 0x6B).all(), "%s slot %d: written past the count" % (name, s)
                if d5[0] == 0:
                    assert exp.tobytes() == kp.tobytes()
        # sd_batch_undistort after firstSeparate: static and dynamic key points; positions inside this workspace's image
        inside = [fc.frame_kps(np.clip(pts[:n, 0], 0, g.W - 1), np.clip(pts[:n, 1] / 2, 0, g.H - 1), s) for s, n in enumerate(counts)]
        ws.set_kps(dict(enumerate(inside)))
        b.set_distortion(fc.TUM1_K4, d5)
        try:
            slots = [3, 0, 2]                                            # slot 1 is not in the call
            b.undistort(list(range(ws.n)))
            b.first_separate(slots, [[(0.0, 0.0, g.W / 2.0, float(g.H))]] * 3, [[7]] * 3)
            b.undistort(slots)
            for s in slots:
                ks, _, _ = b.download(s); kd = b.download_dynamic(s)[0]
                assert len(ks) + len(kd) == counts[s] and (len(kd) > 0 or counts[s] == 1), "slot %d: %d static, %d dynamic" % (s, len(ks), len(kd))
                assert b.download_keys_un(s).tobytes() == undistorted(orc, ks, fc.TUM1_K4, d5).tobytes(), "%s slot %d static" % (name, s)
                assert b.download_dynamic_keys_un(s).tobytes() == undistorted(orc, kd, fc.TUM1_K4, d5).tobytes(), "%s slot %d dynamic" % (name, s)
            assert b.download_keys_un(1).tobytes() == undistorted(orc, inside[1], fc.TUM1_K4, d5).tobytes()
        finally:
            b.set_distortion(fc.TUM1_K4, Z5)


# ---- cvtColor
@pytest.fixture(scope="module")
def triple_gray(orc):
    """The gray image of the 4096 x 4096 image of all triples, per channel order, once."""
    img = fc.all_triples(3)
    return {rgb: orc.cvt_gray(img, rgb) for rgb in (1, 0)}


@pytest.mark.parametrize("channels,rgb", [(3, 1), (3, 0), (4, 1), (4, 0)])
def test_cvt_gray_every_triple(fe, gpu, triple_gray, channels, rgb):
    import torch
    src = fc.all_triples(channels)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.zeros((4096, 4096), dtype=torch.uint8, device="cuda")
    fe.cvt_gray_device(d_src.data_ptr(), 4096, 4096, 4096 * channels, 4096 * 4096 * channels, channels, rgb, d_dst.data_ptr(), 4096, 4096 * 4096, 1)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    bad = np.nonzero(got != triple_gray[rgb])
    assert len(bad[0]) == 0, "%d triples differ, first %r: %d vs %d" % (len(bad[0]), src[bad[0][0], bad[1][0]], got[bad[0][0], bad[1][0]], triple_gray[rgb][bad[0][0], bad[1][0]])


@pytest.mark.parametrize("channels,rgb", [(3, 1), (3, 0), (4, 1), (4, 0)])
def test_cvt_gray_sizes_strides_and_offsets(fe, gpu, orc, channels, rgb):
    """Widths around the 16-pixel and 4-pixel paths, padded strides and pitches, base pointers 1 - 3 bytes off, three images: the whole
    destination buffer, pads and guard bytes included, equals the expectation."""
    import torch
    guard = 64
    for w in fc.CVT_WIDTHS:
        for h in fc.CVT_HEIGHTS:
            rng = np.random.default_rng([w, h, channels])
            imgs = fc.cvt_images(w, h, channels)
            so, do = 1 + (w + h) % 3, 1 + (w + 2 * h) % 3
            ss, ds = w * channels + 5, w + 3
            sp, dp = ss * h + 7, ds * h + 5
            src = np.concatenate([rng.integers(0, 256, so, dtype=np.uint8), fc.padded(imgs.reshape(3, h, w * channels), ss, sp, lambda k: rng.integers(0, 256, k), tail=guard)])
            dst0 = rng.integers(0, 256, guard + do + 3 * dp + guard, dtype=np.uint8)
            exp = dst0.copy()
            for i in range(3):
                v = exp[guard + do + i * dp:guard + do + i * dp + ds * h].reshape(h, ds)
                v[:, :w] = orc.cvt_gray(imgs[i], rgb)
            outs = []
            for flip in ([False, True] if channels == 4 else [False]):
                s = src.copy()
                if flip:                                                  # the 4th channel must not matter
                    for i in range(3):
                        v = s[so + i * sp:so + i * sp + ss * h].reshape(h, ss)
                        v[:, 3:4 * w:4] ^= 0xFF
                d_src = torch.from_numpy(s).cuda(); d_dst = torch.from_numpy(dst0).cuda()
                fe.cvt_gray_device(d_src.data_ptr() + so, w, h, ss, sp, channels, rgb, d_dst.data_ptr() + guard + do, ds, dp, 3)
                torch.cuda.synchronize()
                outs.append(d_dst.cpu().numpy())
            for got in outs:
                bad = np.nonzero(got != exp)[0]
                assert len(bad) == 0, "%d x %d: %d bytes differ, first at %d (image area starts at %d, pitch %d, stride %d)" % (w, h, len(bad), bad[0], guard + do, dp, ds)


# ---- depth conversion and Hamming
def test_depth_to_f32_every_value_and_sizes(fe, gpu, orc):
    import torch
    sent = F32(-123.5)
    cases = [(fc.all_u16()[None], f) for f in fc.DEPTH_FACTORS]
    for w in fc.DEPTH_WIDTHS:
        for h in fc.DEPTH_HEIGHTS:
            cases.append((np.random.default_rng([w, h]).integers(0, 65536, (3, h, w), dtype=np.uint16), fc.DEPTH_FACTORS[(w + h) % 4]))
    for k, (imgs, f) in enumerate(cases):
        n, h, w = imgs.shape
        ss = w + (0 if k < 4 else 3); sp = ss * h + (0 if k < 4 else 5)
        src = fc.padded(imgs, ss, sp, 40000, tail=8)
        d_src = torch.from_numpy(src.view(np.int16)).cuda()
        d_dst = torch.full((n * h * w + 16,), float(sent), dtype=torch.float32, device="cuda")
        fe.depth_to_f32_device(d_src.data_ptr(), w, h, ss, f, d_dst.data_ptr(), n, sp)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        exp = np.concatenate([orc.depth_to_f32(im, f).reshape(-1) for im in imgs])
        assert eq(got[:len(exp)], exp), "%d x %d x %d factor %r" % (n, w, h, f)
        assert (got[len(exp):] == sent).all()


def test_hamming_matrix_sizes_and_every_distance(fe, gpu):
    import torch
    seen = set()
    for a, b, planted in fc.hamming_sets():
        na, nb = len(a), len(b)
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        out = torch.full((na * nb + 16,), -16657, dtype=torch.int16, device="cuda")
        fe.hamming_matrix_device(da.data_ptr(), na, db.data_ptr(), nb, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        ref = fc.np_hamming(a, b)
        assert np.array_equal(got[:na * nb].view(np.uint16).reshape(na, nb), ref), "%d x %d" % (na, nb)
        assert (got[na * nb:] == -16657).all(), "%d x %d: written past na * nb" % (na, nb)
        assert fe.DescriptorDistance(a[0], b[0]) == ref[0, 0]
        seen.update(int(v) for v in ref.reshape(-1))
    assert set(range(257)) <= seen
