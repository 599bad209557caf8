"""GPU parity of sd_batch_search_for_triangulation / sd_batch_create_new_map_points with the sequential CPU oracle
(tests/cpp/triangulate_oracle.cpp): every crafted case of triangulate_cases.py, the threshold scans, the shapes at which the kernels
take another path and a seeded random sweep, all byte for byte -- match arrays, pair lists, counts and the sd_new_map_point records
including the f32 bits of xw."""
import numpy as np
import pytest

import triangulate_cases as tc

pytestmark = pytest.mark.gpu
SLOTS = 48


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = tc.Workspace(fe, SLOTS, tc.vocabulary(synth, 5))
    yield w
    w.close()


@pytest.fixture(scope="module")
def vocs(synth, orc):
    out = {}
    for seed in (5, 6):
        voc = tc.vocabulary(synth, seed)
        out[seed] = (voc, orc.Vocabulary.from_nodes(voc))
    return out


def use(ws, fe, voc):
    ws.V.close()
    ws.V = fe.Vocabulary.from_nodes(voc)


def check_search(ws, pairs, only_stereo=False, check_orientation=False, lv=None, shared=None):
    """pairs: [(kf1, kf2)] with FeatureVectors attached; one device call, every pair against the oracle.  shared = (kfs, [(a, b)]):
    pairs given as indices into a list of keyframes that share slots."""
    if shared is None:
        kfs = [k for p in pairs for k in p]
        idx = [(2 * p, 2 * p + 1) for p in range(len(pairs))]
    else:
        kfs, idx = shared
    ws.upload(kfs)
    h1 = ws.has_table([kfs[a] for a, _ in idx]); h2 = ws.has_table([kfs[b] for _, b in idx])
    ws.b.search_for_triangulation([a for a, _ in idx], [b for _, b in idx], [kfs[a]["Tcw"] for a, _ in idx], [kfs[b]["Tcw"] for _, b in idx], tc.CAM,
                                  d_has_mp1=h1.data_ptr() if h1 is not None else None, d_has_mp2=h2.data_ptr() if h2 is not None else None,
                                  only_stereo=only_stereo, checkOrientation=check_orientation)
    total = 0
    for p, (a, b) in enumerate(idx):
        o = tc.search(kfs[a], kfs[b], lv=lv or ws.lv, only_stereo=only_stereo, check_orientation=check_orientation)
        m, pr, nm = ws.b.download_matches(p)
        n1 = len(kfs[a]["kp"])
        assert nm == o["nmatches"], "pair %d: nmatches %d vs %d" % (p, nm, o["nmatches"])
        assert np.array_equal(m[:n1], o["match"]) and np.all(m[n1:] == -1), "pair %d: match array" % p
        assert pr.tobytes() == o["pairs"].tobytes(), "pair %d: vMatchedPairs" % p
        total += nm
    return total


def check_create(ws, cases, lv=None):
    """One sd_batch_create_new_map_points call for all the cases (they agree on having median depths); every keyframe against the oracle."""
    kfs, kf_idx, off, nb_idx, med = [], [], [0], [], []
    for c in cases:
        kf_idx.append(len(kfs)); kfs.append(c["kf1"])
        for k, nb in enumerate(c["neighbours"]):
            nb_idx.append(len(kfs)); kfs.append(nb)
            if c["median_depth"] is not None:
                med.append(c["median_depth"][k])
        off.append(len(nb_idx))
    mono = cases[0]["median_depth"] is not None
    assert all((c["median_depth"] is not None) == mono for c in cases)
    ws.upload(kfs)
    hk = ws.has_table([kfs[i] for i in kf_idx]); hn = ws.has_table([kfs[i] for i in nb_idx]) if nb_idx else None
    ws.b.create_new_map_points(kf_idx, [kfs[i]["Tcw"] for i in kf_idx], off, nb_idx, [kfs[i]["Tcw"] for i in nb_idx] or np.zeros((0, 16), np.float32), tc.CAM,
                               neigh_median_depth=med if mono else None, d_kf_has_mp=hk.data_ptr() if hk is not None else None,
                               d_neigh_has_mp=hn.data_ptr() if hn is not None else None)
    total = 0
    for k, c in enumerate(cases):
        o = tc.create(c["kf1"], c["neighbours"], c["median_depth"], lv=lv or ws.lv)["new"]
        g = ws.b.download_new_map_points(k)
        assert len(g) == len(o), "%s: nnew %d vs %d" % (c["name"], len(g), len(o))
        assert g.tobytes() == o.tobytes(), "%s: the new map points differ" % c["name"]
        total += len(o)
    return total


def scenes(vocs, seed0, shapes, median=False, lv=None):
    voc, O = vocs[5]
    out = []
    for j, (n, k) in enumerate(shapes):
        c = tc.random_scene(voc, seed0 + j, n, k, median=median, lv=lv)
        tc.attach_bow([c["kf1"]] + c["neighbours"], O)
        out.append(c)
    return out


@pytest.mark.parametrize("only_stereo,ori", [(False, False), (False, True), (True, False)])
def test_matcher_cases(ws, fe, synth, vocs, only_stereo, ori):
    """Every crafted matcher case in one call: all the branches of one pair (dist 50 / 51, the tie, the epipolar test beating the
    distance, the epipole exclusion, has_mp on either side, two idx1 on one idx2, a node of REGF + 1 features), identical poses
    (F12 = 0), N = 0 on either side, N = 1, no shared node; with the rotation histogram and with bOnlyStereo."""
    voc, cases = tc.matcher_cases(synth)
    use(ws, fe, voc)
    for c in cases:
        tc.attach_bow([c["kf1"]] + c["neighbours"], vocs[5][1])
    # the FeatureVectors the device computes are the oracle's
    ws.upload([cases[0]["kf1"], cases[0]["neighbours"][0]])
    for s, kf in enumerate((cases[0]["kf1"], cases[0]["neighbours"][0])):
        g = ws.b.download_bow(s)
        assert np.array_equal(g["fv_node"], kf["fv"][0]) and np.array_equal(g["fv_feature"], kf["fv"][1])
    big = np.bincount(np.unique(cases[0]["neighbours"][0]["fv"][0], return_inverse=True)[1]).max()
    assert big == tc.REGF + 1, "one node of KF2 holds the register path's size + 1"
    n = check_search(ws, [(c["kf1"], c["neighbours"][0]) for c in cases], only_stereo, ori)
    assert n >= 1


@pytest.mark.parametrize("n_pairs", [1, 2, 17])
def test_pairs_per_call(ws, fe, vocs, n_pairs):
    """1, 2 and 17 pairs in one call, over keyframes that share slots (a slot is KF1 of one pair and KF2 of another)."""
    use(ws, fe, vocs[5][0])
    c = scenes(vocs, 20 + n_pairs, [(90, 5)])[0]
    kfs = [c["kf1"]] + c["neighbours"]
    idx = [((3 * p) % 6, (3 * p + 1 + p // 6) % 6) for p in range(n_pairs)]
    idx = [(a, b if b != a else (b + 1) % 6) for a, b in idx]
    n = check_search(ws, None, shared=(kfs, idx))
    assert n > 5 * n_pairs


def test_creation_cases(ws, fe, synth, vocs):
    """The crafted keyframe with one feature per triangulation branch and four neighbours, zero neighbours, and a neighbour skipped by
    the stereo rule: one call, three keyframes.  Then the monocular rule in a call of its own."""
    voc, cases = tc.creation_cases(synth)
    use(ws, fe, voc)
    for c in cases:
        tc.attach_bow([c["kf1"]] + c["neighbours"], vocs[6][1])
    by = {c["name"]: c for c in cases}
    assert check_create(ws, [by["nonrigid_w0"]]) == 0, "x3D[3] == 0: nothing is created (and no NaN point gets through)"
    assert check_create(ws, [by["branches"], by["zero_neighbours"], by["stereo_rule"], by["nonrigid_w0"]]) > 8
    assert check_create(ws, [by["mono_rule"]]) == 1


@pytest.mark.parametrize("kind", tc.SCAN_KINDS)
def test_threshold_scans(ws, fe, vocs, kind):
    """512 pairs in 1-ulp steps across the bound (8 geometries): a contracted or re-associated expression on the device shows here."""
    voc, O = vocs[6]
    use(ws, fe, voc)
    c = tc.scan_case(voc, O, kind, 512)
    if kind == "epipolar":
        n = check_search(ws, [(c["kf1"], c["neighbours"][0])])
    else:
        n = check_create(ws, [c])
    assert 0 < n < 512


@pytest.mark.parametrize("seed,shapes,median,at_least", [(53, [(80, 0), (80, 1), (80, 10)], False, 40), (61, [(60, 20)], True, 30),
                                                         (51, [(70, 10)], False, 40), (45, [(70, 1)], True, 10)])
def test_neighbour_counts(ws, fe, vocs, seed, shapes, median, at_least):
    """n_kf of 1 and 3 with 0, 1, 10 and 20 neighbours, stereo / RGB-D and monocular baseline rule."""
    use(ws, fe, vocs[5][0])
    n = check_create(ws, scenes(vocs, seed, shapes, median=median))
    assert n >= at_least


def test_keyframe_filled_to_capacity(ws, fe, vocs):
    """Keyframe and neighbours hold kp_capacity features: the last rows of every per-slot table are in use."""
    use(ws, fe, vocs[5][0])
    c = scenes(vocs, 60, [(ws.cap, 2)])[0]
    assert len(c["kf1"]["kp"]) == ws.cap
    assert check_create(ws, [c]) > 20
    assert check_search(ws, [(c["kf1"], c["neighbours"][0])]) > 20


def test_distorted_camera_unprojects_the_raw_key_points(gpu, fe, vocs):
    """A workspace with a distortion: mvKeysUn (computed by the device) differs from mvKeys.  The matcher and the tests read mvKeysUn,
    UnprojectStereo reads mvKeys (KeyFrame.cc:620-621); the oracle gets both arrays."""
    w = tc.Workspace(fe, 8, vocs[5][0])
    try:
        w.b.set_distortion([tc.CAM["fx"], tc.CAM["fy"], tc.CAM["cx"], tc.CAM["cy"]], [-0.004, 0.0, 0.0, 0.0, 0.0])
        c = scenes(vocs, 75, [(200, 5)])[0]
        kfs = [c["kf1"]] + c["neighbours"]
        w.upload(kfs)
        w.b.undistort(list(range(len(kfs))))
        moved = 0.0
        for s, k in enumerate(kfs):
            k["kp_raw"] = k["kp"]
            k["kp"] = w.b.download_keys_un(s)
            assert len(k["kp"]) == len(k["kp_raw"])
            moved = max(moved, float(np.abs(k["kp"]["x"] - k["kp_raw"]["x"]).max()))
        assert moved > 0.5, "the undistorted key points must differ from the raw ones"
        hk = w.has_table([c["kf1"]]); hn = w.has_table(c["neighbours"])
        w.b.create_new_map_points([0], [c["kf1"]["Tcw"]], [0, 5], [1, 2, 3, 4, 5], [k["Tcw"] for k in c["neighbours"]], tc.CAM,
                                   d_kf_has_mp=hk.data_ptr() if hk is not None else None, d_neigh_has_mp=hn.data_ptr() if hn is not None else None)
        o = tc.create(c["kf1"], c["neighbours"], lv=w.lv)
        unprojected = [t for t in o["trace"] if tc.PATHS[t["path"]] in ("unproject1", "unproject2") and tc.OUTCOMES[t["outcome"]] == "created"]
        assert len(unprojected) >= 3, "the scene must create points through UnprojectStereo"
        assert w.b.download_new_map_points(0).tobytes() == o["new"].tobytes()
    finally:
        w.close()


def test_twelve_levels(gpu, fe, synth, vocs):
    """An extractor with SD_MAX_LEVELS levels: the level tables are used to their end."""
    g = dict(tc.GEOM, nlevels=12)
    w = tc.Workspace(fe, 8, vocs[5][0], g)
    try:
        c = scenes(vocs, 70, [(120, 4)], lv=w.lv)[0]
        assert int(c["kf1"]["kp"]["octave"].max()) == 11
        assert check_create(w, [c]) > 10
        assert check_search(w, [(c["kf1"], c["neighbours"][1])], check_orientation=True) > 5
    finally:
        w.close()


def test_random_sweep(ws, fe, vocs):
    """24 keyframe-neighbour pairs of synthetic two-view scenes, mixed stereo and mono points, 0.5 px noise: byte-equal.  18 pairs under
    the stereo / RGB-D baseline rule, 6 under the monocular one."""
    use(ws, fe, vocs[5][0])
    assert check_create(ws, scenes(vocs, 80, [(200, 6), (160, 6), (220, 6)])) > 100
    assert check_create(ws, scenes(vocs, 90, [(150, 6)], median=True)) > 20


def test_second_call_with_other_sizes(ws, fe, vocs):
    """The same workspace, a larger call and then a smaller one (and the matcher in between): stale tables would show."""
    use(ws, fe, vocs[5][0])
    big = scenes(vocs, 100, [(200, 8), (150, 3)])
    small = scenes(vocs, 110, [(40, 1)])
    assert check_create(ws, big) > 40
    check_search(ws, [(big[0]["kf1"], big[0]["neighbours"][0]), (small[0]["kf1"], small[0]["neighbours"][0])])
    n_small = check_create(ws, small)
    assert n_small < 40
    assert check_create(ws, big[1:]) > 10


def test_errors(ws, fe, vocs):
    import ctypes as C
    use(ws, fe, vocs[5][0])
    c = scenes(vocs, 120, [(30, 1)])[0]
    ws.upload([c["kf1"], c["neighbours"][0]])
    b, T = ws.b, [c["kf1"]["Tcw"], c["neighbours"][0]["Tcw"]]

    def code(f):
        with pytest.raises(fe.SdError) as e:
            f()
        return e.value.code

    assert code(lambda: b.search_for_triangulation([0], [SLOTS], T[:1], T[1:], tc.CAM)) == fe.SD_ERR_INVALID          # slot out of range
    assert code(lambda: b.search_for_triangulation([-1], [1], T[:1], T[1:], tc.CAM)) == fe.SD_ERR_INVALID
    assert code(lambda: b.search_for_triangulation([], [], np.zeros((0, 16)), np.zeros((0, 16)), tc.CAM)) == fe.SD_ERR_INVALID      # n_pairs = 0
    L, cam, i32 = fe.lib(), fe.camera_array(tc.CAM), np.zeros(4, np.int32)
    T16 = np.ascontiguousarray(np.stack(T), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sd_batch_search_for_triangulation(b.h, -3, vp(i32), vp(i32), vp(T16), vp(T16), vp(cam), None, None, 0, 0, None) == fe.SD_ERR_INVALID
    assert L.sd_batch_search_for_triangulation(b.h, SLOTS + 1, vp(i32), vp(i32), vp(T16), vp(T16), vp(cam), None, None, 0, 0, None) == fe.SD_ERR_INVALID
    assert L.sd_batch_create_new_map_points(b.h, -1, vp(i32), vp(T16), None, vp(i32), vp(i32), vp(T16), None, None, vp(cam), None, None, None) == fe.SD_ERR_INVALID
    assert L.sd_batch_create_new_map_points(b.h, 0, vp(i32), vp(T16), None, vp(i32), vp(i32), vp(T16), None, None, vp(cam), None, None, None) == fe.SD_ERR_INVALID
    assert code(lambda: b.create_new_map_points([0], T[:1], [0, 1], [SLOTS + 3], T[1:], tc.CAM)) == fe.SD_ERR_INVALID
    off = np.array([1, 2], np.int32)                                                                                    # offsets must start at 0
    assert L.sd_batch_create_new_map_points(b.h, 1, vp(i32), vp(T16), None, vp(off), vp(i32), vp(T16), None, None, vp(cam), None, None, None) == fe.SD_ERR_INVALID
    # a slot that holds a frame but no bag of words: extraction resets nothing here, so take a fresh workspace
    w = tc.Workspace(fe, 2, vocs[5][0])
    try:
        assert code(lambda: w.b.search_for_triangulation([0], [1], T[:1], T[1:], tc.CAM)) == fe.SD_ERR_STATE
        assert code(lambda: w.b.create_new_map_points([0], T[:1], [0, 1], [1], T[1:], tc.CAM)) == fe.SD_ERR_STATE
        w.upload([c["kf1"]])                                                                                            # BoW on slot 0 only
        assert code(lambda: w.b.search_for_triangulation([0], [1], T[:1], T[1:], tc.CAM)) == fe.SD_ERR_STATE
        assert code(lambda: w.b.download_new_map_points(0)) == fe.SD_ERR_INVALID                                        # nothing created yet
    finally:
        w.close()
    # after the errors the workspace still works
    assert check_search(ws, [(c["kf1"], c["neighbours"][0])]) >= 0
