"""GPU parity of the dynamic-object cull: firstSeparate, Separate (BF cross-check + classifyH/F), UpdateFrame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _frames(synth, orc, cfg, seq, ts):
    out = []
    for t in ts:
        rgb, depth, _ = synth.rgbd_frame(seq, t, cfg)
        out.append((orc.cvt_gray(rgb, 1), depth))
    return out


def _boxes(synth, cfg, seq, t, extra):
    rows = synth.boxes_for_frame(seq, t, cfg)
    rects = synth.rows_to_rects(rows)
    return np.concatenate([rects, extra]) if len(extra) else rects


@pytest.fixture(scope="module", params=[0, 5000, -5000],
                ids=["settings", "5000-features-one-box-over-2048", "5000-features-then-a-smaller-workspace"])
def scene(request, gpu, fe, orc, synth):
    """params: 0 = the settings file's nFeatures (2000); 5000 = an extractor that yields more than 2048 key points per image AND a box that holds more
    than 2048 of them in both frames -- the reference has no bound here (Frame.cc:555-604 and Tracking.cc:1093-1239 work on std::vectors); rounds 1-3
    refused it (SD_ERR_UNSUPPORTED), since round 4 the key-point tables of k_box_separate / k_separate are sized by the workspace and a box's train
    descriptors pass through LDS in chunks.  -5000: the 5000-feature workspace, then a smaller one created after it and kept alive while the large
    one runs -- the kernels' dynamic-LDS limits only ever grow, a later, smaller workspace must not lower them."""
    import torch
    cfg = dict(synth.KITTI03_RGBD)
    big = request.param != 0
    if big:
        cfg["n_features"] = abs(request.param)
    ts = [0, 3]
    fr = _frames(synth, orc, cfg, 8, ts)
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], 3)
    small = None
    if request.param < 0:
        s = synth.KITTI03_RGBD
        small = fe.Batch(fe.ORBextractor(s["n_features"], s["scale_factor"], s["n_levels"], s["ini_th_fast"], s["min_th_fast"]),
                         s["width"], s["height"], 1)
    b.extract_host(np.stack([g for g, _ in fr]))
    factor = float(np.float32(1.0) / np.float32(cfg["depth_map_factor"]))
    d_dev = torch.from_numpy(np.stack([d for _, d in fr]).view(np.int16)).cuda()
    b.rgbd_from_u16(d_dev.data_ptr(), cfg["width"], cfg["width"] * cfg["height"], 2, factor, cfg["bf"])
    # boxes: the 3 synthetic ones + one EMPTY box (flat border region has no corners inside a 2x2 box) in the
    # middle of the list (triggers the erase quirk) + one box overlapping box 0 (keypoints in two boxes)
    per_frame = []
    for t in ts:
        base = _boxes(synth, cfg, 8, t, np.zeros((0, 4)))
        empty = np.array([[0.25, 0.25, 1.5, 1.5]])
        overlap = base[0:1] + np.array([[20., 10., 0., 0.]])
        boxes = np.concatenate([base[:1], empty, base[1:], overlap] + ([np.array([[60., 30., 1100., 320.]])] if big else []))
        idx = np.arange(len(boxes), dtype=np.int32) + 10
        per_frame.append((boxes, idx))
    # oracle side
    ref = []
    for (g, d), (boxes, idx) in zip(fr, per_frame):
        o = orc.Extractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
        kp, desc = o(g)
        ur, dep = orc.stereo_from_rgbd(kp, orc.depth_to_f32(d, factor), cfg["bf"])
        r = orc.first_separate(kp, desc, boxes, idx, np.zeros(len(boxes), np.uint8), np.zeros((len(boxes), 2)))
        r["ur"] = ur[r["perm"]]; r["dep"] = dep[r["perm"]]
        ref.append(r)
    b.first_separate([0, 1], [p[0] for p in per_frame], [p[1] for p in per_frame])
    if big:
        for r in ref:
            assert r["Ns"] + r["Nd"] > 2048 and np.diff(r["boxStart"]).max() > 2048, "the big case must put more than 2048 key points into one box (%d, %d)" % (r["Ns"] + r["Nd"], np.diff(r["boxStart"]).max())
    yield dict(b=b, cfg=cfg, ref=ref, ts=ts)
    b.close()
    if small is not None:
        small.close()


def test_first_separate(scene, fe):
    b = scene["b"]
    for slot, r in enumerate(scene["ref"]):
        g = b.download_boxes(slot)
        assert r["Nd"] > 50, "the synthetic boxes must contain keypoints"
        assert g["n_static"] == r["Ns"] and g["n_all"] == r["Ns"] + r["Nd"]
        assert g["nb"] == len(r["boxes"]) and np.array_equal(g["boxes"], r["boxes"]) and np.array_equal(g["box_idx"], r["box_idx"])
        # device lists index the dynamic arrays; the oracle's index the concatenated (static ++ dynamic) arrays
        assert np.array_equal(g["boxStart"], r["boxStart"]) and np.array_equal(g["boxItems"] + r["Ns"], r["boxItems"])
        assert (g["box_status"] == -1).all()
        kp, desc, _ = b.download(slot)
        Ns = r["Ns"]
        assert len(kp) == Ns and kp.tobytes() == r["kp"][:Ns].tobytes() and np.array_equal(desc, r["desc"][:Ns])   # N = N_s
        ur, dep = b.download_rgbd(slot)
        assert np.array_equal(ur[:Ns].view(np.uint32), r["ur"][:Ns].view(np.uint32))
        assert np.array_equal(dep[:Ns].view(np.uint32), r["dep"][:Ns].view(np.uint32))
        dk, dd, dur, ddep = b.download_dynamic(slot)
        assert dk.tobytes() == r["kp"][Ns:].tobytes(), "dynamic keypoints (class_id = original index)"
        assert np.array_equal(dd, r["desc"][Ns:])
        assert np.array_equal(dur.view(np.uint32), r["ur"][Ns:].view(np.uint32)) and np.array_equal(ddep.view(np.uint32), r["dep"][Ns:].view(np.uint32))
        # a keypoint inside two boxes is listed in both
        items = g["boxItems"]
        assert len(items) > len(np.unique(items))


def _similarity_H(cfg, dt):
    # synth.cut_frame: x_t = (x_0 + 3t - cx) * s^t + cx  ->  x_cur = a * x_ref + bx (ref = t0, cur = t0 + dt)
    s = 1.01 ** dt
    a = s
    bx = (3.0 * dt - cfg["cx"]) * s + cfg["cx"]      # for t0 = 0
    by = (-cfg["cy"]) * s + cfg["cy"]
    return np.array([[a, 0, bx], [0, a, by], [0, 0, 1]], np.float32)


@pytest.mark.parametrize("flag", [1, 2])
def test_separate_and_update_frame(scene, fe, orc, flag):
    b, cfg, ref = scene["b"], scene["cfg"], scene["ref"]
    cur, rf = ref[1], ref[0]
    if flag == 1:
        M = _similarity_H(cfg, scene["ts"][1] - scene["ts"][0])           # points_cur = H21 * points_ref
    else:
        # a fundamental matrix compatible with that similarity: F = [e]x H with the epipole at the principal point
        H = _similarity_H(cfg, scene["ts"][1] - scene["ts"][0]).astype(np.float64)
        e = np.array([cfg["cx"], cfg["cy"], 1.0])
        ex = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
        M = (ex @ H).astype(np.float32)
    last_idx = [np.array([10, 12, 13], np.int32)]
    last_status = [np.array([0, 2, -1], np.int32)]
    cur_boxes = b.download_boxes(1)
    oret, osc, ods, odyn, omt = orc.separate(M, flag, dict(kp=cur["kp"], desc=cur["desc"], boxStart=cur["boxStart"],
                                                           boxItems=cur["boxItems"], box_idx=cur["box_idx"]),
                                             dict(kp=rf["kp"], desc=rf["desc"], boxStart=rf["boxStart"], boxItems=rf["boxItems"],
                                                  box_idx=rf["box_idx"]),
                                             last_idx[0], last_status[0], cur_boxes["box_status"])
    b.separate([1], [0], M[None], [flag], last_idx, last_status)
    ret, ds, dyn, mt = b.download_separate(0)
    nb = len(cur["box_idx"])
    assert len(omt) > 20, "boxes should produce cross-checked matches"
    assert ret == oret
    assert np.array_equal(ds[:nb + 1], ods) and np.array_equal(mt, omt) and np.array_equal(dyn, odyn)
    assert np.array_equal(b.download_boxes(1)["box_status"], osc)
    # UpdateFrame
    n_before = int(b.counts(2)[1])
    app = orc.update_frame(cur["kp"], cur["boxStart"], cur["boxItems"], ods, odyn)
    b.update_frame(only_if_static=False)
    n_after = int(b.counts(2)[1])
    assert n_after == n_before + len(app)
    kp, desc, _ = b.download(1)
    exp_kp = np.concatenate([cur["kp"][:cur["Ns"]], cur["kp"][app]]); exp_desc = np.concatenate([cur["desc"][:cur["Ns"]], cur["desc"][app]])
    assert kp.tobytes() == exp_kp.tobytes() and np.array_equal(desc, exp_desc)
    ur, dep = b.download_rgbd(1)
    assert np.array_equal(ur[:n_after].view(np.uint32), np.concatenate([cur["ur"][:cur["Ns"]], cur["ur"][app]]).view(np.uint32))
    # restore N = N_s for the next parametrisation (the dynamic arrays and box lists are untouched by UpdateFrame)
    _truncate(b, fe, 1, cur["Ns"])


def _truncate(b, fe, slot, n):
    import torch
    kp_p, desc_p, cnt_p, cap = b.results_device()
    t = fe.as_torch_u8(cnt_p + 4 * slot, 4)
    t.copy_(torch.from_numpy(np.array([n], np.int32).view(np.uint8)).cuda())
    torch.cuda.synchronize()


def test_randomised_cull_configurations(gpu):
    """6 fixed draws of tools/fuzz_cull.py (random box sets incl. empty / overlapping / partly outside boxes, H or F exact or
    perturbed, random carried-over states): firstSeparate, Separate and UpdateFrame identical to the oracle.  (70 draws were
    run when written: 26 of 34 Separate calls re-admitted their boxes, 25 box-status changes, 19 empty boxes dropped.)"""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("fuzz_cull", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_cull.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    assert m.run(6, 17) == 0


# ---- crafted key points, boxes and models (tests/cull_cases.py): the images only make the slots valid, key points and descriptors are
# written over the extraction results.  tests/test_oracle_cull.py pins which branch every case reaches (and that the threshold scans can see
# an FMA contraction); here the device output on the same arrays must be the oracle's bytes.

import cull_cases as cc  # noqa: E402


def _assert_cases(orc, ws, cases, what, only_if_static=False):
    got = cc.run_cases(ws, cases, only_if_static)
    bad, n_kp, n_dyn = [], 0, 0
    for p, (c, g_) in enumerate(zip(cases, got)):
        o = cc.oracle(orc, c, only_if_static)
        d = cc.compare(g_, o, orc)
        n_kp += len(c["cur"]["kp"]) + len(c["ref"]["kp"]); n_dyn += len(o["dyn"])
        if d:
            bad.append("%s [pair %d of %d]: %s" % (c["name"], p, len(cases), "; ".join(d)))
    print("%s: %d cases, %d key points, %d classified matches compared, %d cases differ" % (what, len(cases), n_kp, n_dyn, len(bad)))
    assert not bad, "\n".join(bad)
    return got


def test_crafted_cases_match_oracle(gpu, fe, orc):
    """cull_cases.suite() in launches of 128 pairs, then the distortion group (its own camera) on the same workspace: every field that
    firstSeparate, Separate and UpdateFrame leave behind is the oracle's.  Building the library with -ffp-contract=fast makes this test fail
    on the threshold_scans cases (test_oracle_cull.py::test_threshold_scans_see_contraction shows the same source deciding 112 / 95 of their
    matches differently when contracted)."""
    cases = cc.suite()
    ws = cc.Workspace(fe, 128)
    try:
        assert ws.cap == cc.GEOM.cap, "kp_capacity %d, the generators assume %d" % (ws.cap, cc.GEOM.cap)
        for k0 in range(0, len(cases), ws.n_pairs):
            _assert_cases(orc, ws, cases[k0:k0 + ws.n_pairs], "suite %d.." % k0)
        _assert_cases(orc, ws, cc.distortion(), "distortion")
        _assert_cases(orc, ws, cases[:3], "after the distortion is switched off again")
    finally:
        ws.close()


def test_crafted_chunk_boundary(gpu, fe, orc):
    """Train lists of 2047, 2048, 2049 and 4097 descriptors: the LDS chunk limit of k_separate, with ties across it."""
    ws = cc.Workspace(fe, 4, cc.GEOM_BIG)
    try:
        assert ws.cap >= 4200, "kp_capacity %d" % ws.cap
        _assert_cases(orc, ws, cc.chunk_boundary(ws.cap), "chunk_boundary")
    finally:
        ws.close()


def _pool():
    S = {c["name"]: c for c in cc.suite()}
    return [S[n] for n in ("threshold_scans-flag1-0", "empty_box_patterns-no_keypoints_cur", "hamming_ties-two_queries_3_259", "empty_box_patterns-none",
                           "membership_edges-depth", "empty_box_patterns-no_keypoints_ref", "threshold_scans-flag2-1", "empty_box_patterns-010010",
                           "partition_sizes-n513-alternating", "status_table-n_last_64", "readmission-shared")]


def test_crafted_cases_do_not_depend_on_slot_or_neighbours(gpu, fe, orc):
    """1, 7, 8, 9, 17 pairs per launch, the pool in rotated order: the same case in different slots, frames without key points and a frame
    without boxes between full ones.  Every case's result is the same bytes in every launch, equals the oracle, and a launch run twice gives
    the same bytes (the LDS atomics are order-free)."""
    pool = _pool()
    ws = cc.Workspace(fe, 17)
    seen = {}
    try:
        for n in (1, 7, 8, 9, 17):
            cases = [pool[(k + n) % len(pool)] for k in range(n)]
            got = _assert_cases(orc, ws, cases, "%d pairs" % n)
            again = cc.run_cases(ws, cases)
            for p, (c, g_, a_) in enumerate(zip(cases, got, again)):
                bts = cc.result_bytes(g_)
                assert bts == cc.result_bytes(a_), "%s [pair %d of %d]: two runs of one launch differ" % (c["name"], p, n)
                assert seen.setdefault(c["name"], bts) == bts, "%s [pair %d of %d]: differs from its result in another launch" % (c["name"], p, n)
        assert len(seen) == len(pool)
    finally:
        ws.close()


def test_update_frame_only_if_static(gpu, fe, orc):
    """UpdateFrame(only_if_static) leaves a frame alone whose Separate returned 0 and re-admits where it returned 1; UpdateFrame(always)
    re-admits the consistent match of the ret-0 box too."""
    cases = cc.readmission()
    ws = cc.Workspace(fe, len(cases))
    try:
        gated = _assert_cases(orc, ws, cases, "only_if_static", only_if_static=True)
        always = _assert_cases(orc, ws, cases, "always", only_if_static=False)
        shared, ret0 = 0, 1
        assert gated[ret0]["ret"] == 0 and gated[ret0]["count_after"] == gated[ret0]["cur"]["n_static"]
        assert always[ret0]["count_after"] == always[ret0]["cur"]["n_static"] + 1
        assert gated[shared]["ret"] == 1 and gated[shared]["count_after"] == always[shared]["count_after"] == gated[shared]["cur"]["n_static"] + 11
    finally:
        ws.close()


def _overflow_frames(cap):
    """Three boxes that each hold every key point; 3 N box items against an item table of 2 * cap: N just above and just below."""
    n_over = 2 * cap // 3 + 1
    n_under = 2 * cap // 3
    assert 3 * n_over > 2 * cap >= 3 * n_under and n_over <= cap
    rng = np.random.default_rng(5)
    out = []
    for n in (n_over, n_under):
        k = cc.kps(rng.uniform(4, cc.W - 4, n), rng.uniform(4, cc.H - 4, n))
        out.append(cc.frame(k, cc.sc.rand_desc(rng, n), [(0.0, 0.0, float(cc.W), float(cc.H))] * 3, [1, 2, 3]))
    return out


def test_item_table_overflow_is_refused(gpu, fe, orc):
    """A frame whose box lists need more than 2 * kp_capacity items: the next synchronisation refuses it and names the box tables; the frame
    just below the limit, alone on a fresh workspace, is the oracle's."""
    ws = cc.Workspace(fe, 1)
    try:
        over, under = _overflow_frames(ws.cap)
        cc.upload(ws, [over, under])
        ws.b.first_separate([0, 1], [over["boxes"], under["boxes"]], [over["ids"], under["ids"]])
        with pytest.raises(fe.SdError) as e:
            ws.b.sync()
        assert e.value.code == fe.SD_ERR_UNSUPPORTED and "box tables" in str(e.value)
    finally:
        ws.close()
    ws = cc.Workspace(fe, 1)
    try:
        cc.upload(ws, [under])
        ws.b.first_separate([0], [under["boxes"]], [under["ids"]])
        r = cc.oracle_frame(orc, under)
        assert r["boxStart"][-1] == 3 * len(under["kp"]) <= 2 * ws.cap
        bad = cc.compare_frame([], "below the limit", cc.download_frame(ws.b, 0), r, np.full(3, -1))
        assert not bad, "; ".join(bad)
    finally:
        ws.close()


def test_item_table_overflow_leaves_an_empty_frame_record(gpu, fe, orc):
    """The tracker enqueues Separate and UpdateFrame behind firstSeparate without a synchronisation between them, so an overflowed frame must
    reach them as a frame without boxes (nb = 0, boxStart[0] = 0): then no index leaves the item table.  Pair 0 has the overflowed frame as
    its current frame, pair 1 as its reference frame, pair 2 is an untouched neighbour; the whole chain is enqueued, the synchronisation
    refuses, and the neighbour's results are the oracle's."""
    ws = cc.Workspace(fe, 3)
    try:
        over, under = _overflow_frames(ws.cap)
        (neighbour, _) = cc.readmission()
        frames = [under, over, over, under, neighbour["ref"], neighbour["cur"]]
        cc.upload(ws, frames)
        b = ws.b
        b.first_separate(list(range(6)), [f["boxes"] for f in frames], [f["ids"] for f in frames])
        b.separate([1, 3, 5], [0, 2, 4], np.stack([cc.I3] * 3), [1, 1, 1], [[], [], []], [[], [], []])
        b.update_frame(only_if_static=False)
        with pytest.raises(fe.SdError) as e:
            b.sync()
        assert e.value.code == fe.SD_ERR_UNSUPPORTED and "box tables" in str(e.value)
        for slot in (1, 2):
            g = b.download_boxes(slot)
            assert g["nb"] == 0 and g["boxStart"].tolist() == [0] and g["n_all"] == len(over["kp"]) and g["n_static"] == 0
        for pair in (0, 1):
            ret, ds, dyn, mt = b.download_separate(pair)
            assert ret == 0 and not ds.any() and len(dyn) == 0
        o = cc.oracle(orc, neighbour)
        ret, ds, dyn, mt = b.download_separate(2)
        assert ret == o["ret"] and np.array_equal(ds[:3], o["dynStart"]) and np.array_equal(dyn, o["dyn"]) and np.array_equal(mt, o["matches"])
        bad = cc.compare_frame([], "neighbour", cc.download_frame(b, 5), dict(o["cur"], Ns=o["cur"]["Ns"]), o["status"])
        # UpdateFrame has run: the static count has grown by the re-admitted key points, everything else is as after Separate
        bad = [m for m in bad if not m.startswith("neighbour static")]
        kp, desc, _ = b.download(5)
        assert not bad and kp.tobytes() == o["kp_after"].tobytes() and np.array_equal(desc, o["desc_after"]), "; ".join(bad)
    finally:
        ws.close()
