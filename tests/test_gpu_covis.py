"""GPU parity of the device covisibility graph (sd_covis_*) with the sequential CPU oracle (tests/cpp/covis_oracle.cpp): every list, its
order, every weight, flag and count.  The crafted cases of covis_cases.py, the shapes at which the kernels take another path, the
independence of the results from insertion order and of a local-map query from its call, keyframes taken from extracted frames, the link
into the device KeyFrameDatabase, the refusals and seeded random maps."""
import numpy as np
import pytest

import covis_cases as cc

pytestmark = pytest.mark.gpu
CASES = cc.crafted_cases()


def check(fe, ops, what, **kw):
    want, br = cc.run_oracle(ops)
    got = cc.run_device(fe, ops, **kw)
    cc.assert_same(got, want, what)
    return want, br


def test_records_are_the_headers(gpu, fe):
    assert fe.COVIS_KF_INFO_DTYPE.itemsize == 36 and fe.COVIS_CULL_DTYPE.itemsize == 12 and fe.COVIS_LOCAL_DTYPE.itemsize == 24


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_cases(gpu, fe, case):
    check(fe, case["ops"], case["name"])
    if any(op[0] == "local" for op in case["ops"]):
        check(fe, case["ops"], case["name"] + " (device arrays)", device=True)


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("n_kf", [1, 2, 63, 64, 65, 1025])
def test_keyframe_counts(gpu, fe, n_kf):
    """Around a wave, the 256 threads of the counter and sort kernels and the 1024 of the scans, the culling walk and the local map."""
    want, _ = check(fe, cc.shape_script(n_kf, 12), "%d keyframes" % n_kf)
    assert len(want[-1]) == n_kf


def bound_script(K):
    """Keyframes up to id K - 1, the counted ones at both ends of the id range."""
    b = cc.Builder()
    for k in range(K):
        b.kf(k, n=40 if k in (0, 1, K - 2, K - 1) else 1)
    b.share(K - 1, 0, 16); b.share(K - 1, K - 2, 15); b.share(0, 1, 3)
    own = [b.point([K - 1]), b.point([0])]
    b.op("update", [K - 1, 0]).op("cull", [K - 1, 0, K - 2], None, True, 0.0).op("parent", [K - 2], [K - 1]).op("local", [own, own[:1]])
    return b.ops


@pytest.mark.parametrize("K", [4096, 4097])
def test_both_sides_of_the_lds_counter_bound(gpu, fe, K):
    """KFcounter and the local map's votes live in LDS up to COVIS_LDS_KEYFRAMES = 4096 keyframe ids and in a global row per job above."""
    assert fe.COVIS_LDS_KEYFRAMES == 4096
    want, _ = check(fe, bound_script(K), "%d keyframes" % K)
    last = want[-1][K - 1]
    assert last[6] == [0, K - 2] and last[7] == [16, 15] and want[1][0][1][:2] == [0, K - 1]


@pytest.mark.parametrize("n_feat", [0, 1, 63, 64, 65, 2000])
def test_feature_counts(gpu, fe, n_feat):
    want, _ = check(fe, cc.shape_script(6, n_feat), "%d features" % n_feat)
    assert want[-1][0][2] == n_feat


@pytest.mark.parametrize("n_obs", [0, 1, 64, 65])
def test_observers_of_one_point(gpu, fe, n_obs):
    want, _ = check(fe, cc.shape_script(66, 20, observers_of_point=n_obs), "%d observers" % n_obs)
    assert len(want[-1][0][8]) == max(n_obs - 1, 0)          # keyframe 0's row: everyone else who sees its points


# ---------------------------------------------------------------- orders that must not matter
def test_insertion_order_does_not_matter(gpu, fe):
    """The index by map point is filled through an atomic cursor: keyframes added and matches set in another order give the same answers."""
    ops = cc.random_script(7, n_kf=30, rounds=2)
    rng = np.random.default_rng(1)
    adds = [op for op in ops if op[0] == "add"]
    first_match = next(i for i, op in enumerate(ops) if op[0] == "match")
    assert all(op[0] == "add" for op in ops[:first_match])
    shuffled = [adds[i] for i in rng.permutation(len(adds))] + list(ops[first_match:])
    for i, op in enumerate(shuffled):
        if op[0] == "match":
            last = {}
            for k, f, m in zip(op[1], op[2], op[3]):
                last[(k, f)] = m                              # the last value of a feature wins, whatever the order of the rest
            items = [(k, f, m) for (k, f), m in last.items()]
            # a point may move between two features of one keyframe inside the list: the refusal looks at the state after the call
            perm = [items[j] for j in rng.permutation(len(items))]
            shuffled[i] = ("match", [x[0] for x in perm], [x[1] for x in perm], [x[2] for x in perm])
    want, _ = cc.run_oracle(ops)
    cc.assert_same(cc.run_device(fe, ops), want, "as written")
    cc.assert_same(cc.run_device(fe, shuffled), want, "shuffled")


def test_a_local_map_query_does_not_depend_on_its_call(gpu, fe):
    ops = cc.random_script(11, rounds=1)
    base = [op for op in ops if op[0] != "local"]
    frames = [op for op in ops if op[0] == "local"][0][1]
    together = cc.run_device(fe, base + [("local", frames)])
    for q, fr in enumerate(frames):
        alone = cc.run_device(fe, base + [("local", [fr])])
        assert alone[-2][0] == together[-2][q], "query %d alone" % q
    cc.assert_same(together, cc.run_oracle(base + [("local", frames)])[0], "together")


# ---------------------------------------------------------------- from extracted frames, and into the KeyFrameDatabase
def test_keyframes_from_extracted_frames(gpu, fe, synth):
    """Two synthetic stereo frames -> ORB -> stereo match -> add (device to device): octave, uRight >= 0 and depth are the slot's."""
    cfg = synth.KITTI_STEREO
    frames = [synth.stereo_frame(seq=4, t=t) for t in range(2)]
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], 4)
    g = fe.CovisibilityGraph(8, 4 * b.cap, 4096, 2, 4096)
    try:
        b.extract_host(np.stack([im for (l, r, _) in frames for im in (l, r)]))
        b.stereo_match(2, cfg["bf"], cfg["fx"])
        g.add(b, [0, 2], [5, 3], [0, 1])
        with pytest.raises(fe.SdError) as e:
            g.add(b, [2], [3])
        assert e.value.code == fe.SD_ERR_STATE
        ops = []
        n = {}
        for slot, kf, frame in ((0, 5, 0), (2, 3, 1)):
            kp = b.download(slot)[0]
            ur, dep, _ = b.download_stereo(frame)
            n[kf] = len(kp)
            assert n[kf] > 100 and np.any(ur[:n[kf]] >= 0) and np.any(ur[:n[kf]] < 0)
            ops.append(("add", kf, kp["octave"].astype(np.uint8), ur[:n[kf]], dep[:n[kf]], kf == 3))
        m = min(n.values())
        idx = np.arange(0, m, 3)
        match = ("match", [5] * len(idx) + [3] * len(idx), list(idx) * 2, list(range(len(idx))) * 2)
        g.set_matches(match[1], match[2], match[3])
        g.update_connections([5, 3])
        cull = g.keyframe_culling([5, 3], None, False, 35.0)
        loc = g.local_map([np.arange(0, len(idx), 2)])
        ops += [match, ("update", [5, 3]), ("cull", [5, 3], None, False, 35.0), ("local", [np.arange(0, len(idx), 2)])]
        want, _ = cc.run_oracle(ops)
        got = [cc.cull_record([(x["flag"], x["n_mps"], x["n_redundant"]) for x in cull]),
               [cc.local_record(x["local_kf"], x["reference_kf"], x["local_points"], x["info"]["n_voted"], x["entry_bad"]) for x in loc],
               [cc.device_conn(g, 3), cc.device_conn(g, 5)]]
        cc.assert_same(got, want, "frames")
        assert want[-1][1][6] == [3] and want[-1][1][4] == 3 and want[-1][0][4] == -1 and want[0][1][0][1] > 0
    finally:
        g.close(); b.close()


def test_set_covisible_from_equals_set_covisible_with_the_downloaded_lists(gpu, fe):
    """Keyframe 0 has twelve neighbours (the ten best go over, ties by id), the others one, keyframe 13 none."""
    bld = cc.Builder()
    bld.kf(0, n=260)
    for k in range(1, 14):
        bld.kf(k, n=24)
    for k in range(1, 13):
        bld.share(0, k, 15 + k // 2)
    ops = bld.op("update", list(range(14))).ops
    K, F, P = cc.max_ids(ops)
    g = fe.CovisibilityGraph(K, F, P, K, F)
    a = fe.KeyFrameDatabase(K, 4 * K, 1, 8); b = fe.KeyFrameDatabase(K, 4 * K, 1, 8)
    try:
        cc.run_device(fe, ops, graph=g)
        ids = cc.ids_of(ops)
        for k in ids:
            a.add_host(k, [k + 1], [1.0]); b.add_host(k, [k + 1], [1.0])
        lists = [g.connections(k)["ordered_id"] for k in ids]
        assert sorted(len(x) for x in lists) == [0] + [1] * 12 + [12]
        a.set_covisible(ids, [x[:10] for x in lists])
        b.set_covisible_from(g, ids)
        for k in ids:
            ea, eb = a.entry(k), b.entry(k)
            assert list(ea["neighbours"]) == list(eb["neighbours"]) == list(lists[ids.index(k)][:10]), "keyframe %d" % k
            assert eb["live"] and eb["seq"] == ea["seq"] and list(eb["word"]) == [k + 1]
        b.erase([ids[0]])
        assert list(b.entry(ids[0])["neighbours"]) == list(lists[0][:10]) and not b.entry(ids[0])["live"]     # an erase leaves the device-written neighbours
        with pytest.raises(fe.SdError) as e:
            b.set_covisible_from(g, [ids[0]])
        assert e.value.code == fe.SD_ERR_STATE
        small = fe.KeyFrameDatabase(K - 1, 8, 1, 8)
        try:
            small.add_host(1, [1], [1.0])
            with pytest.raises(fe.SdError) as e:
                small.set_covisible_from(g, [1])              # the graph's ids do not fit the database
            assert e.value.code == fe.SD_ERR_INVALID
        finally:
            small.close()
    finally:
        a.close(); b.close(); g.close()


# ---------------------------------------------------------------- matches from device arrays
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_cases_with_matches_from_device_arrays(gpu, fe, case):
    check(fe, case["ops"], case["name"] + " (device matches)", device_matches=True)


@pytest.mark.parametrize("seed", (3, 4))
def test_device_matches_equal_host_matches(gpu, fe, seed):
    ops = cc.random_script(200 + seed)
    host = cc.run_device(fe, ops)
    cc.assert_same(cc.run_device(fe, ops, device_matches=True, device=True), host, "seed %d" % seed)
    cc.assert_same(host, cc.run_oracle(ops)[0], "seed %d against the oracle" % seed)


def test_device_matches_are_checked_on_the_device(gpu, fe):
    """What the host-array path refuses before a launch, the device path reports with the next download: an item out of range is left
    out (reported once), two features of one keyframe naming one point until the tables are corrected."""
    z8, zf = np.zeros(4, np.uint8), np.zeros(4, np.float32)
    g = fe.CovisibilityGraph(4, 16, 6, 2, 16)
    try:
        g.add_host(1, z8, zf - 1, zf + 1); g.add_host(2, z8, zf - 1, zf + 1)
        g.set_matches_device([1, 2, 3, 1, 1, 5, -1], [0, 0, 0, 4, 1, 0, 0], [2, 2, 2, 2, 6, 2, 2])      # keyframe 3 not live, feature 4, point 6, ids 5 and -1
        g.update_connections([1])
        with pytest.raises(fe.SdError) as e:
            g.connections(1)
        assert e.value.code == fe.SD_ERR_INVALID
        c = g.connections(1)                                  # reported once; the two good items went in
        assert list(c["ordered_id"]) == [2] and list(c["ordered_weight"]) == [1]
        g.set_matches_device([1], [1], [2])                   # features 0 and 1 of keyframe 1 name point 2
        g.update_connections([1])
        for _ in range(2):
            with pytest.raises(fe.SdError) as e:
                g.connections(1)
            assert e.value.code == fe.SD_ERR_INVALID
        with pytest.raises(fe.SdError) as e:
            g.keyframe_culling([1, 2], None, True, 0.0)
        assert e.value.code == fe.SD_ERR_INVALID
        g.set_matches([1], [1], [-1])                         # corrected, through the host path
        g.update_connections([1])
        assert list(g.connections(1)["ordered_weight"]) == [1]
        g.set_matches([1, 1], [2, 3], [4, 4])                 # the host path no longer knows the tables: the device finds this one too
        g.update_connections([1])
        with pytest.raises(fe.SdError) as e:
            g.local_map([[2]])
        assert e.value.code == fe.SD_ERR_INVALID
        g.clear()                                             # the host knows the tables again and refuses before a launch
        g.add_host(1, z8, zf - 1, zf + 1)
        with pytest.raises(fe.SdError) as e:
            g.set_matches([1, 1], [2, 3], [4, 4])
        assert e.value.code == fe.SD_ERR_INVALID
        g.update_connections([1])
        assert g.connections(1)["live"]
    finally:
        g.close()


# ---------------------------------------------------------------- refusals
def test_refusals(gpu, fe):
    z8, zf = np.zeros(4, np.uint8), np.zeros(4, np.float32)
    for args in ((0, 8, 8, 1, 8), (fe.COVIS_MAX_KEYFRAMES + 1, 8, 8, 1, 8), (4, 0, 8, 1, 8), (4, 8, 0, 1, 8), (4, 8, 8, 0, 8), (4, 8, 8, 1, 0)):
        with pytest.raises(fe.SdError) as e:
            fe.CovisibilityGraph(*args)
        assert e.value.code == fe.SD_ERR_INVALID
    g = fe.CovisibilityGraph(4, 10, 6, 2, 3)
    try:
        g.add_host(1, z8, zf - 1, zf + 1)
        g.add_host(2, z8, zf - 1, zf + 1)
        for bad, code in ((lambda: g.add_host(1, z8[:1], zf[:1], zf[:1]), fe.SD_ERR_STATE),                 # live id added again
                          (lambda: g.add_host(4, z8[:1], zf[:1], zf[:1]), fe.SD_ERR_INVALID),               # id outside [0, max_keyframes)
                          (lambda: g.add_host(3, z8[:3], zf[:3], zf[:3]), fe.SD_ERR_CAPACITY),              # 8 + 3 > 10 pool features
                          (lambda: g.set_matches([1, 1], [0, 1], [2, 2]), fe.SD_ERR_INVALID),               # two features, one point
                          (lambda: g.set_matches([3], [0], [2]), fe.SD_ERR_STATE),                          # not in the graph
                          (lambda: g.set_matches([1], [4], [2]), fe.SD_ERR_INVALID),                        # feature index outside the keyframe
                          (lambda: g.set_matches([1], [0], [6]), fe.SD_ERR_INVALID),                        # point id outside [0, max_points)
                          (lambda: g.set_point_bad([6]), fe.SD_ERR_INVALID),
                          (lambda: g.set_parent([1], [3]), fe.SD_ERR_STATE),                                # a parent that was never added
                          (lambda: g.set_parent([1], [4]), fe.SD_ERR_INVALID),
                          (lambda: g.update_connections([1, 2, 1]), fe.SD_ERR_CAPACITY),                    # three jobs, max_jobs = 2
                          (lambda: g.update_connections([3]), fe.SD_ERR_STATE),
                          (lambda: g.keyframe_culling([1, 1]), fe.SD_ERR_INVALID),                          # a candidate twice
                          (lambda: g.local_map([[0], [0], [0]]), fe.SD_ERR_CAPACITY)):
            with pytest.raises(fe.SdError) as e:
                bad()
            assert e.value.code == code
        assert fe.lib().sd_covis_download_culling(g.h, None, 0, None) == fe.SD_ERR_STATE
        assert fe.lib().sd_covis_download_local_map(g.h, 0, None, None, 0, None, 0) == fe.SD_ERR_STATE
        # the refused calls left the graph as it was: a point may move between two features of a keyframe inside one call
        g.set_matches([1, 1, 2, 2, 2, 2], [0, 1, 0, 1, 2, 3], [2, 3, 2, 3, 4, 5])
        g.set_matches([1, 1], [2, 0], [2, -1])
        g.update_connections([1])
        c = g.connections(1)
        assert list(c["ordered_id"]) == [2] and list(c["ordered_weight"]) == [2] and c["parent"] == 2
    finally:
        g.close()


def test_local_point_overflow_is_an_error_not_a_short_list(gpu, fe):
    g = fe.CovisibilityGraph(4, 16, 8, 1, 3)
    try:
        z8, zf = np.zeros(4, np.uint8), np.zeros(4, np.float32)
        g.add_host(1, z8, zf - 1, zf + 1); g.add_host(2, z8, zf - 1, zf + 1)
        g.set_matches([1, 1, 2, 2, 2], [0, 1, 0, 1, 2], [0, 1, 0, 1, 2])
        r = g.local_map([[0]])
        assert list(r[0]["local_kf"]) == [1, 2] and list(r[0]["local_points"]) == [0, 1, 2]        # exactly max_local_points
        g.set_matches([2], [3], [3])
        with pytest.raises(fe.SdError) as e:
            g.local_map([[0]])
        assert e.value.code == fe.SD_ERR_CAPACITY
        info = np.zeros(1, fe.COVIS_LOCAL_DTYPE)
        assert fe.lib().sd_covis_download_local_map(g.h, 0, info.ctypes.data_as(fe.C.c_void_p), None, 0, None, 0) == fe.SD_ERR_CAPACITY
        assert info[0]["overflow"] == 1 and info[0]["n_points"] == 4
        g.clear()
        assert not g.connections(1)["live"]
        g.add_host(1, z8, zf - 1, zf + 1)
        assert g.connections(1)["live"] and g.local_map([[0]])[0]["reference_kf"] == -1
    finally:
        g.close()


# ---------------------------------------------------------------- random maps
@pytest.mark.parametrize("seed", range(8))
def test_random_maps(gpu, fe, seed):
    """40 keyframes x 60 features over four rounds of matches, bad flags, updates in two calls, culling, local maps, erases and parents."""
    ops = cc.random_script(100 + seed)
    want, br = cc.run_oracle(ops)
    cc.assert_same(cc.run_device(fe, ops, device=bool(seed & 1)), want, "seed %d" % seed)
    assert br["cu_flagged"] > 0 and br["ac_changed"] > 0 and br["er_connection"] > 0 and br["lm_parent_break"] > 0
