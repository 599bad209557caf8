"""CPU side of proj_cases.py: the `_ex` entries of the oracle agree with the plain ones; every named case of both projection
matchers leaves the reference where it was built to (the exit is read from the `_ex` outcome AND from a numpy restatement of the whole
function that shares no code with the oracle); every outcome is reached; the best / second-best patterns produce the distances and
levels they were written for; every scan window flips exactly once; check_domain refuses what lies outside the contract, before
anything is uploaded."""
import numpy as np
import pytest

import area_cases as ac
import proj_cases as pc


@pytest.fixture(scope="module")
def ff_scenes():
    return pc.ff_scenes()


@pytest.fixture(scope="module")
def lm_scenes():
    return pc.lm_scenes()


def _same_as_numpy_ff(orc, P, th, bMono, ori=True, mpd=False):
    o = pc.oracle_ff(orc, P, th, bMono, ori, mpd); n = pc.np_search_by_projection(P, th, bMono, ori, mpd)
    assert [pc.FF_OUTCOMES[c] for c in o["outcome"]] == n["outcome"], P["name"]
    pc.same_ff(o, n, P["name"] + " oracle vs numpy")
    return o


def _same_as_numpy_lm(orc, F, th, nn, lim):
    o = pc.oracle_lm(orc, F, th, nn, lim); n = pc.np_search_local_map(F, th, nn, lim)
    assert [pc.LM_OUTCOMES[c] for c in o["outcome"]] == n["outcome"], F["name"]
    pc.same_lm(o, n, F["name"] + " oracle vs numpy")
    assert np.array_equal(o["best"], n["best"]), F["name"]
    return o


def test_outcome_names_are_the_oracles(orc):
    assert orc.FF_NAMES == pc.FF_OUTCOMES and orc.LM_NAMES == pc.LM_OUTCOMES


def test_ex_entries_agree_with_the_plain_ones_on_a_crafted_scene(orc, ff_scenes, lm_scenes):
    for sc in ff_scenes:
        for P in sc["pairs"]:
            cur, last = P["cur"], P["last"]
            occ = P["occupied"] if len(P["occupied"]) else None
            m, pr, nm = orc.search_by_projection(cur["kp"], cur["desc"], cur["ur"], last["kp"], last["desc"], P["xw"], P["flags"], P["Tcw"], P["Tlw"],
                                                 ac.cam_array(), pc.LV.scale, sc["th"], sc["bMono"], True, occupied=occ)
            pc.same_ff(dict(match=m, pairs=pr, nm=nm), pc.oracle_ff(orc, P, sc["th"], sc["bMono"]), P["name"])
    sc = lm_scenes[1]
    for F in sc["frames"]:
        fr = F["frame"]
        tr, pm, km, nm = orc.search_local_map(fr["kp"], fr["desc"], fr["ur"], np.ascontiguousarray(F["points"]).view(orc.MAP_POINT_DTYPE), F["pdesc"], F["Tcw"],
                                              ac.cam_array(), pc.LV.scale, sc["th"], sc["nnratio"], sc["cos_limit"], occupied=F["occupied"] if len(F["occupied"]) else None)
        pc.same_lm(dict(track=tr, mp_match=pm, kp_match=km, nm=nm), pc.oracle_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"]), F["name"])


def test_ex_entries_agree_with_the_plain_ones_on_extracted_frames(orc, synth, pkg):
    """The frames test_gpu_match.py / test_gpu_localmap.py build (synthetic KITTI stereo, sequence 5), here through the oracle's own
    extractor: frame t against frame t - 1, and frame 1 against the stereo points of frame 0 as its local map."""
    cfg = synth.KITTI_STEREO
    cam10 = pkg.frontend.camera_array(pkg.frontend.make_camera(cfg))
    ref = []
    for t in range(2):
        l, r, _ = synth.stereo_frame(seq=5, t=t)
        oL = orc.Extractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
        oR = orc.Extractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
        kL, dL = oL(l); kR, dR = oR(r)
        ur, dep, _, _ = orc.stereo_matches(oL, oR, kL, dL, kR, dR, cfg["bf"], cfg["fx"])
        ref.append(dict(kp=kL, desc=dL, ur=ur, depth=dep, scale=oL.scale.copy()))
    I = np.eye(4, dtype=np.float32)
    rng = np.random.default_rng(5)
    cur, last = ref[1], ref[0]
    xw, valid = orc.unproject(last["kp"], last["depth"], cam10, I)
    fl = valid | (((rng.random(len(valid)) < 0.6) & (valid > 0)).astype(np.uint8) << 1)
    occ = (rng.random(len(cur["kp"])) < 0.05).astype(np.uint8)
    Tcw = I.copy(); Tcw[2, 3] = -0.8
    args = (cur["kp"], cur["desc"], cur["ur"], last["kp"], last["desc"], xw, fl, Tcw, I, cam10, cur["scale"], 15.0, False, True)
    m, pr, nm = orc.search_by_projection(*args, occupied=occ)
    m2, pr2, nm2, out = orc.search_by_projection_ex(*args, occupied=occ)
    assert nm == nm2 > 50 and np.array_equal(m, m2) and np.array_equal(pr, pr2)
    h = pc.histogram(out, orc.FF_NAMES)
    assert h["matched"] == nm and h["matched"] + h.get("matched_then_culled", 0) == len(pr) and sum(h.values()) == len(last["kp"])
    idx = np.nonzero(valid)[0]
    pts = np.zeros(len(idx), orc.MAP_POINT_DTYPE)
    pts["xw"] = xw[idx]; d = np.linalg.norm(xw[idx].astype(np.float64), axis=1)
    pts["normal"] = (xw[idx] / d[:, None]).astype(np.float32); pts["max_distance"] = d * 1.2 ** last["kp"]["octave"][idx]
    pts["min_distance"] = pts["max_distance"] / np.float32(1.2 ** 7); pts["flags"] = 3
    args = (cur["kp"], cur["desc"], cur["ur"], pts, last["desc"][idx], Tcw, cam10, cur["scale"], 3.0, 0.8, 0.5)
    tr, pm, km, nm = orc.search_local_map(*args, occupied=occ)
    tr2, pm2, km2, nm2, out, best = orc.search_local_map_ex(*args, occupied=occ)
    assert nm == nm2 > 50 and tr.tobytes() == tr2.tobytes() and np.array_equal(pm, pm2) and np.array_equal(km, km2)
    h = pc.histogram(out, orc.LM_NAMES)
    assert h["matched"] == nm and sum(h.values()) == len(pts)
    assert np.all((best[:, 0] <= pc.TH_HIGH) == np.isin(out, [orc.LM_NAMES.index("matched"), orc.LM_NAMES.index("ratio")]))


def test_frame_frame_cases_take_the_exit_they_are_named_for(orc, ff_scenes):
    reached, ncases = set(), 0
    for sc in ff_scenes:
        pc.check_domain(sc)
        for P in sc["pairs"]:
            for ori in (True, False):
                for mpd in (False, True):
                    o = _same_as_numpy_ff(orc, P, sc["th"], sc["bMono"], ori, mpd)
                    if ori and not mpd:
                        res = o
            names = [pc.FF_OUTCOMES[c] for c in res["outcome"]]
            reached |= set(names)
            chosen = {int(a): int(b) for a, b in res["pairs"]}
            for case, i, outcome, kp in P["cases"]:
                if outcome is None:
                    continue
                ncases += 1
                assert names[i] == outcome, "%s / %s: left at %s, built for %s" % (P["name"], case, names[i], outcome)
                if outcome == "matched":
                    assert chosen[i] == kp, "%s / %s: key point %d, built for %d" % (P["name"], case, chosen[i], kp)
                elif outcome != "matched_then_culled":
                    assert i not in chosen
    assert reached == set(pc.FF_OUTCOMES), "never reached: %r" % (set(pc.FF_OUTCOMES) - reached)
    assert ncases > 300


def test_frame_frame_cases_hold_what_their_names_say(orc, ff_scenes):
    by = {P["name"]: (sc, P) for sc in ff_scenes for P in sc["pairs"]}
    # the level modes come from tlc.z alone
    for mode, want in (("forward", "forward"), ("backward", "backward"), ("between", "between"), ("equal_mb", "between")):
        sc, P = by["ff_level_" + mode]
        assert pc.level_mode(P["Tcw"], P["Tlw"], False) == want and pc.level_mode(P["Tcw"], P["Tlw"], True) == "between"
    assert pc.tlc_z(by["ff_level_equal_mb"][1]["Tcw"], pc.I4) == pc.CAM["mb"]
    sc, P = by["ff_posed"]
    assert not np.array_equal(P["Tcw"], pc.I4) and not np.array_equal(P["Tlw"], pc.I4)
    # bounds: the projection is ON the bound, in f32
    sc, P = by["ff_bounds"]
    u, v, invz, _ = pc.project_f32(P["Tcw"], P["xw"])
    at = {c[0]: c[1] for c in P["cases"]}
    assert u[at["u_eq_minx"]] == pc.CAM["mnMinX"] and u[at["u_eq_maxx"]] == pc.CAM["mnMaxX"]
    assert v[at["v_eq_miny"]] == pc.CAM["mnMinY"] and v[at["v_eq_maxy"]] == pc.CAM["mnMaxY"]
    assert u[at["u_past_minx"]] < 0 and u[at["u_past_maxx"]] > pc.CAM["mnMaxX"] and v[at["v_past_miny"]] < 0 and v[at["v_past_maxy"]] > pc.CAM["mnMaxY"]
    assert np.isposinf(u[at["z_zero_plus"]]) and np.isneginf(u[at["z_zero_minus"]])
    # the radius, independently: area_cases' walk and in_radius
    kp = P["cur"]["kp"]
    for octave in (0, 7):
        r = np.float32(pc.TH_FF) * pc.LV.scale[octave]
        for axis in "xy":
            i_on, i_in = at["radius_%s_oct%d_on" % (axis, octave)], at["radius_%s_oct%d_inside" % (axis, octave)]
            for i, want in ((i_on, 0), (i_in, 1)):
                w = ac.walk(kp, u[i], v[i], r)
                assert len(w["order"]) >= 1 and int(ac.in_radius(kp, w["order"], u[i], v[i], r).sum()) == want
    # the second descriptor array changes matches
    a = pc.oracle_ff(orc, P, sc["th"], False, True, False); b = pc.oracle_ff(orc, P, sc["th"], False, True, True)
    assert not np.array_equal(a["match"], b["match"]) and a["pairs"].tobytes() != b["pairs"].tobytes()
    # the histogram cull clears a key point whose owner survives
    sc, P = by["ff_hist_cull_clears_owner"]
    o = pc.oracle_ff(orc, P, sc["th"], False)
    at = {c[0]: c[1] for c in P["cases"]}
    assert [at["cull_clears.b"], P["cleared"]] in o["pairs"].tolist() and o["match"][P["cleared"]] == -1 and o["nm"] == len(o["pairs"]) - 1
    assert pc.oracle_ff(orc, P, sc["th"], False, check_orientation=False)["match"][P["cleared"]] == at["cull_clears.b"]
    # the counts the order pairs were built for
    assert [len(by[n][1]["last"]["kp"]) for n in ("ff_order0", "ff_order1", "ff_order63", "ff_order64", "ff_order65", "ff_order70")] == [0, 1, 63, 64, 65, 70]
    assert len(by["ff_cur_empty"][1]["cur"]["kp"]) == 0


def test_local_map_cases_take_the_exit_they_are_named_for(orc, lm_scenes):
    reached, ncases = set(), 0
    for sc in lm_scenes:
        pc.check_domain(sc)
        sizes = []
        for F in sc["frames"]:
            o = _same_as_numpy_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"])
            names = [pc.LM_OUTCOMES[c] for c in o["outcome"]]
            reached |= set(names)
            sizes.append(len(F["points"]))
            for case, m, outcome, kp, extra in F["cases"]:
                ncases += 1
                assert names[m] == outcome, "%s / %s: left at %s, built for %s" % (F["name"], case, names[m], outcome)
                assert o["mp_match"][m] == (kp if outcome == "matched" else -1), "%s / %s" % (F["name"], case)
                if "level" in extra:
                    assert o["track"]["level"][m] == extra["level"], "%s / %s: level %d" % (F["name"], case, o["track"]["level"][m])
                if "best" in extra:
                    assert tuple(o["best"][m]) == tuple(extra["best"]), "%s / %s: best / second %r, written for %r" % (F["name"], case, o["best"][m], extra["best"])
        assert set(sizes) >= {0, 1, 63, 64, 65}
        # ON the bounds, in f32
        F = sc["frames"][0]
        at = {c[0]: c[1] for c in F["cases"]}
        u, v, _, _ = pc.project_f32(F["Tcw"], F["points"]["xw"])
        assert u[at["u_eq_minx"]] == 0 and u[at["u_eq_maxx"]] == pc.CAM["mnMaxX"] and v[at["v_eq_miny"]] == 0 and v[at["v_eq_maxy"]] == pc.CAM["mnMaxY"]
        p = F["points"]
        for which, f in (("min", 0.8), ("max", 1.2)):
            m = at["dist_%s_on" % which]
            dist = np.float32(np.sqrt(sum(float(c) * float(c) for c in p["xw"][m])))
            assert np.float32(f) * p["%s_distance" % which][m] == dist
        t = pc.oracle_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"])["track"]
        assert t["view_cos"][at["cos_limit_on"]] == np.float32(sc["cos_limit"]) and t["in_view"][at["cos_limit_on"]] == 1
        F = [f for f in sc["frames"] if f["name"].startswith("lm_order64")][0]
        m = {c[0]: c[1] for c in F["cases"]}["cos_eq_998f"]
        vc = pc.oracle_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"])["track"]["view_cos"][m]
        assert vc == np.float32(0.998) and float(vc) > 0.998, "above 0.998 in f64, equal to it in f32"
    assert reached == set(pc.LM_OUTCOMES), "never reached: %r" % (set(pc.LM_OUTCOMES) - reached)
    assert ncases > 500


def test_second_best_is_not_the_second_smallest():
    """The hand-written table of PATTERNS against a literal run of the reference's loop on the distances alone."""
    for pat, (bp, sp) in pc.PATTERNS.items():
        b1 = b2 = 256; i1 = i2 = -1
        for n, d in enumerate(pat):
            if d < b1:
                b2, b1, i2, i1 = b1, d, i1, n
            elif d < b2:
                b2, i2 = d, n
        assert (i1, i2) == (bp, sp), pat


@pytest.mark.parametrize("kind", pc.FF_SCANS + pc.LM_SCANS)
def test_scan_windows_flip_exactly_once(orc, kind):
    sc, where, variant = pc.scan_scene(orc, kind)
    pc.check_domain(sc)
    assert len(where) == 512 and max(len(o.get("last", o.get("frame"))["kp"]) for o in sc.get("pairs", sc.get("frames"))) <= pc.CAP
    ok = pc.scan_accepted(orc, sc, where)
    for w in range(pc.SCAN_WINDOWS):
        a = ok[variant == w]
        assert len(a) == 32 and a.any() and not a.all(), "%s window %d: the oracle must both accept and reject" % (kind, w)
        assert int(np.abs(np.diff(a.astype(np.int8))).sum()) == 1, "%s window %d: more than one flip" % (kind, w)
    if "pairs" in sc:
        for P in sc["pairs"]:
            _same_as_numpy_ff(orc, P, sc["th"], sc["bMono"])
    else:
        for F in sc["frames"]:
            _same_as_numpy_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"])


def test_refusal_scenes_are_what_they_claim(orc):
    for n, occ, want in ((65, 64, 1), (63, 63, 0), (64, 64, 0)):
        P = pc.ff_refusal_pair(n, occ)
        o = _same_as_numpy_ff(orc, P, pc.TH_FF, False)
        u, v, _, _ = pc.project_f32(P["Tcw"], P["xw"])
        w = ac.walk(P["cur"]["kp"], u[0], v[0], np.float32(pc.TH_FF))
        assert int(ac.in_radius(P["cur"]["kp"], w["order"], u[0], v[0], np.float32(pc.TH_FF)).sum()) == n and int(P["occupied"].sum()) == occ
        assert int((o["pairs"][:, 0] == 0).sum()) == want
        if want:                       # the match is the one free member: the FARTHEST descriptor, beyond the 64 the device keeps
            j = int(o["pairs"][o["pairs"][:, 0] == 0][0, 1])
            d = ac.hamming(P["last"]["desc"][0], P["cur"]["desc"][:n])
            assert not P["occupied"][j] and d[j] == d.max() == 64
    for n, occ, want in ((65, 64, 1), (64, 64, 0), (65, 0, 1)):
        F = pc.lm_refusal_frame(n, occ)
        o = _same_as_numpy_lm(orc, F, pc.REFUSAL_TH_LM, 0.8, 0.5)
        assert int(o["mp_match"][0] >= 0) == want and int(F["occupied"].sum()) == occ


@pytest.mark.parametrize("seed", [0, 1])
def test_random_scenes_numpy_equals_oracle(orc, seed):
    sc = pc.random_ff_scene(seed); pc.check_domain(sc)
    for P in sc["pairs"]:
        o = _same_as_numpy_ff(orc, P, sc["th"], sc["bMono"])
        assert o["nm"] > 10
    sc = pc.random_lm_scene(seed); pc.check_domain(sc)
    for F in sc["frames"]:
        o = _same_as_numpy_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"])
        assert o["nm"] > 10


def test_seeds_depend_on_the_case_alone():
    a = pc.ff_order_pairs(); b = pc.ff_bounds_pair(); c = pc.ff_order_pairs(); d = pc.ff_bounds_pair()
    for x, y in zip(a + [b], c + [d]):
        assert x["cur"]["kp"].tobytes() == y["cur"]["kp"].tobytes() and x["cur"]["desc"].tobytes() == y["cur"]["desc"].tobytes() and x["xw"].tobytes() == y["xw"].tobytes()
    assert pc.random_lm_scene(3)["frames"][1]["pdesc"].tobytes() == pc.random_lm_scene(3)["frames"][1]["pdesc"].tobytes()


class _Untouchable:
    """A workspace that must not be reached: any use of it fails the test."""
    cap, n = pc.CAP, 8

    def __getattr__(self, name):
        raise AssertionError("the workspace was touched (%s) before the domain check" % name)


def test_check_domain_refuses_and_nothing_outside_it_is_uploaded():
    import copy
    good = pc.ff_bounds_pair(); pc.check_domain(good)
    frame = pc.lm_scenes()[0]["frames"][1]; pc.check_domain(frame)
    bad = []
    P = copy.deepcopy(good); P["xw"][3, 1] = np.inf; bad.append(P)                       # non-finite world position
    P = copy.deepcopy(good); P["cur"]["kp"]["x"][2] = np.nan; bad.append(P)              # non-finite key point
    P = copy.deepcopy(good); P["cur"]["ur"][2] = np.nan; bad.append(P)
    P = copy.deepcopy(good); P["Tcw"][0, 3] = np.nan; bad.append(P)
    P = copy.deepcopy(good); P["cur"]["kp"]["octave"][0] = pc.NLEVELS; bad.append(P)     # an octave outside the level set
    P = copy.deepcopy(good); P["last"]["kp"]["octave"][0] = -1; bad.append(P)
    bad.append(pc.nan_projection_pair())                                                 # zc == 0 on the axis: 0 * inf
    big = pc.PairB("too_many", step=40)
    for k in range(pc.CAP + 1):
        big.cur.add(10.0 + (k % 60) * 10, 10.0 + (k // 60) * 10, np.zeros(32, np.uint8))
    bad.append(big.build())                                                              # more key points than the capacity
    for P in bad:
        with pytest.raises(ValueError, match="outside the domain"):
            pc.check_domain(P)
        with pytest.raises(ValueError, match="outside the domain"):
            pc.device_ff(_Untouchable(), dict(name="bad", th=pc.TH_FF, bMono=False, pairs=[P]))
    badf = []
    F = copy.deepcopy(frame); F["points"]["xw"][1, 0] = np.nan; badf.append(F)
    F = copy.deepcopy(frame); F["points"]["normal"][1, 0] = np.inf; badf.append(F)
    F = copy.deepcopy(frame); F["points"]["max_distance"][1] = np.nan; badf.append(F)
    F = copy.deepcopy(frame); F["frame"]["kp"]["octave"][1] = 9; badf.append(F)
    F = copy.deepcopy(frame); F["points"]["xw"][1] = pc.cam_centre(F["Tcw"]); F["points"]["flags"][1] = 3; badf.append(F)       # viewCos = 0 / 0
    B = pc.LocalB("lm_nan"); B.point(xw=[0.0, 0.1, 0.0], normal=[0.0, 0.0, 1.0], max_distance=1.0); badf.append(B.build())
    for F in badf:
        with pytest.raises(ValueError, match="outside the domain"):
            pc.check_domain(F)
        with pytest.raises(ValueError, match="outside the domain"):
            pc.device_lm(_Untouchable(), dict(name="bad", th=1.0, nnratio=0.8, cos_limit=0.5, frames=[F]))
    with pytest.raises(ValueError, match="outside the domain"):
        pc.upload(_Untouchable(), [bad[1]["cur"]])
