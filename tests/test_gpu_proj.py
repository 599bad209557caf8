"""GPU parity of the two projection matchers of Tracking -- k_proj_candidates / k_proj_resolve and k_local_candidates / k_local_resolve --
with the CPU oracle on the crafted inputs of proj_cases.py, byte for byte and without a tolerance: the named decision cases, the 1-ulp
scans the oracle placed, the truncated-list refusals (flags 4 and 64 of sd_batch_sync), seeded random scenes, and the independence of a
result from its slot and its neighbours in the launch.  test_proj_cases.py shows on the CPU that the inputs hold what they claim.
Every test prints one summary line per scene (run with -s): pairs or frames, points compared, named cases, the oracle's outcome histogram."""
import numpy as np
import pytest

import fuse_cases as fc
import proj_cases as pc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = fc.Workspace(fe, 8, tc.vocabulary(synth, 5))
    assert w.cap >= pc.CAP and w.lv.scale.tobytes() == pc.LV.scale.tobytes()
    yield w
    w.close()


def _summary(sc, wants, names):
    objs = sc.get("pairs", sc.get("frames"))
    out = np.concatenate([w["outcome"] for w in wants]) if wants else np.zeros(0, np.int32)
    print("\n[proj] %-22s %s %d, points %d, key points %d, named cases %d, outcomes %r" % (
        sc["name"], "pairs" if "pairs" in sc else "frames", len(objs), len(out), sum(len(o.get("cur", o.get("frame"))["kp"]) for o in objs),
        sum(len(o["cases"]) for o in objs), pc.histogram(out, names)))


def check_ff(ws, orc, sc, check_orientation=True, use_mpdesc=False):
    got = pc.device_ff(ws, sc, check_orientation=check_orientation, use_mpdesc=use_mpdesc)
    wants = [pc.oracle_ff(orc, P, sc["th"], sc["bMono"], check_orientation, use_mpdesc) for P in sc["pairs"]]
    _summary(sc, wants, pc.FF_OUTCOMES)
    for P, g, w in zip(sc["pairs"], got, wants):
        pc.same_ff(g, w, "%s / %s%s%s" % (sc["name"], P["name"], "" if check_orientation else " (no orientation check)", " (d_mp_desc)" if use_mpdesc else ""))
    return wants


def check_lm(ws, orc, sc):
    got = pc.device_lm(ws, sc)
    wants = [pc.oracle_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"]) for F in sc["frames"]]
    _summary(sc, wants, pc.LM_OUTCOMES)
    for F, g, w in zip(sc["frames"], got, wants):
        pc.same_lm(g, w, "%s / %s" % (sc["name"], F["name"]))
    return wants


@pytest.fixture(scope="module")
def ff_scenes():
    return {s["name"]: s for s in pc.ff_scenes()}


@pytest.mark.parametrize("name", ["ff_geometry", "ff_mono", "ff_order", "ff_orientation"])
def test_frame_frame_named_cases(ws, orc, ff_scenes, name):
    wants = check_ff(ws, orc, ff_scenes[name])
    assert sum(w["nm"] for w in wants) > 0


def test_frame_frame_without_the_orientation_check(ws, orc, ff_scenes):
    for name in ("ff_orientation", "ff_geometry"):
        check_ff(ws, orc, ff_scenes[name], check_orientation=False)


def test_frame_frame_with_a_separate_descriptor_array(ws, orc, ff_scenes):
    """d_mp_desc points at descriptors that differ from the last frame's key-point descriptors where it changes matches; then without it."""
    sc = ff_scenes["ff_geometry"]
    a = check_ff(ws, orc, sc, use_mpdesc=True)
    b = check_ff(ws, orc, sc, use_mpdesc=False)
    assert a[0]["pairs"].tobytes() != b[0]["pairs"].tobytes()


@pytest.mark.parametrize("which", [0, 1])
def test_local_map_named_cases(ws, orc, which):
    wants = check_lm(ws, orc, pc.lm_scenes()[which])
    assert sum(w["nm"] for w in wants) > 200


@pytest.mark.parametrize("kind", pc.FF_SCANS)
def test_frame_frame_scans(ws, orc, kind):
    sc, where, variant = pc.scan_scene(orc, kind)
    wants = check_ff(ws, orc, sc)
    assert 0 < sum(int((w["outcome"] == pc.FF_OUTCOMES.index("matched")).sum()) for w in wants) < 512


@pytest.mark.parametrize("kind", pc.LM_SCANS)
def test_local_map_scans(ws, orc, kind):
    sc, where, variant = pc.scan_scene(orc, kind)
    wants = check_lm(ws, orc, sc)
    assert 0 < sum(int((w["outcome"] == pc.LM_OUTCOMES.index("matched")).sum()) for w in wants) < 512


def _refused(fe, flag, run):
    with pytest.raises(fe.SdError) as e:
        run()
    assert e.value.code == fe.SD_ERR_UNSUPPORTED and "(flag %d)" % flag in str(e.value), str(e.value)


def test_frame_frame_truncated_list_refusals(ws, orc, fe, ff_scenes):
    """65 hits with the nearest 64 occupied: the reference matches the 65th, the kept 64 run out -> flag 4, never "no match".  63 hits, all
    occupied: the oracle's "no match", no error.  64 hits, all occupied: the list may be the head of a longer one -> the oracle's bytes or
    the refusal, nothing else.  After every refusal a valid call on the same workspace equals the oracle (the flag was cleared)."""
    sc = dict(name="ff_refusal_65", th=pc.TH_FF, bMono=False, pairs=[pc.ff_refusal_pair(65, 64)])
    assert pc.oracle_ff(orc, sc["pairs"][0], sc["th"], False)["nm"] == 2
    _refused(fe, 4, lambda: pc.device_ff(ws, sc))
    check_ff(ws, orc, ff_scenes["ff_mono"])
    check_ff(ws, orc, dict(name="ff_refusal_63", th=pc.TH_FF, bMono=False, pairs=[pc.ff_refusal_pair(63, 63)]))
    sc = dict(name="ff_refusal_64", th=pc.TH_FF, bMono=False, pairs=[pc.ff_refusal_pair(64, 64)])
    try:
        check_ff(ws, orc, sc)
        print("\n[proj] 64 hits, all occupied: the device answered with the oracle's bytes")
    except fe.SdError as e:
        assert e.code == fe.SD_ERR_UNSUPPORTED and "(flag 4)" in str(e), str(e)
        print("\n[proj] 64 hits, all occupied: the device refused (flag 4)")
        check_ff(ws, orc, ff_scenes["ff_mono"])


def test_local_map_truncated_list_refusals(ws, orc, fe):
    mk = lambda n, occ: dict(name="lm_refusal_%d_%d" % (n, occ), th=pc.REFUSAL_TH_LM, nnratio=0.8, cos_limit=0.5, frames=[pc.lm_refusal_frame(n, occ)])
    sc = mk(65, 64)
    assert pc.oracle_lm(orc, sc["frames"][0], sc["th"], 0.8, 0.5)["nm"] == 2
    _refused(fe, 64, lambda: pc.device_lm(ws, sc))
    check_lm(ws, orc, mk(64, 64))              # overflow is 0: the oracle's "no match", no error (and the flag was cleared)
    check_lm(ws, orc, mk(65, 0))               # a truncated list whose first two entries are free decides like the full one


@pytest.mark.parametrize("seed", range(8))
def test_random_scenes(ws, orc, seed):
    wants = check_ff(ws, orc, pc.random_ff_scene(seed))
    assert sum(w["nm"] for w in wants) > 50
    wants = check_lm(ws, orc, pc.random_lm_scene(seed))
    assert sum(w["nm"] for w in wants) > 50


def test_local_map_scratch_grows_with_a_larger_second_call(gpu, fe, synth, orc):
    """A fresh workspace: one frame with one point, then two frames with a few hundred points, then the first call again."""
    w = fc.Workspace(fe, 2, tc.vocabulary(synth, 5))
    try:
        B = pc.LocalB("lm_growth_one")
        B.simple("only")
        small = dict(name="lm_growth_small", th=3.0, nnratio=0.8, cos_limit=0.5, frames=[B.build()])
        big = pc.random_lm_scene(1, n_frames=2)
        assert sum(len(F["points"]) for F in big["frames"]) > 200
        assert check_lm(w, orc, small)[0]["nm"] == 1
        check_lm(w, orc, big)
        assert check_lm(w, orc, small)[0]["nm"] == 1
    finally:
        w.close()


def test_frame_frame_result_is_independent_of_slot_and_neighbours(ws, orc, ff_scenes):
    """The same pair as pair 0 of 1, and as pair 3 of 5 on other slots with an empty pair before it: the same bytes."""
    order = {P["name"]: P for P in ff_scenes["ff_order"]["pairs"]}
    P, A, B, E = order["ff_order63"], order["ff_order70"], ff_scenes["ff_orientation"]["pairs"][1], order["ff_order0"]
    E = dict(E, cur=dict(E["cur"], kp=E["cur"]["kp"][:0], desc=E["cur"]["desc"][:0], ur=E["cur"]["ur"][:0], depth=E["cur"]["depth"][:0]), occupied=E["occupied"][:0])
    sc = dict(name="ff_alone", th=pc.TH_FF, bMono=False, pairs=[P])
    alone = pc.device_ff(ws, sc)[0]
    want = pc.oracle_ff(orc, P, sc["th"], False)
    pc.same_ff(alone, want, "pair 0 of 1")
    pc.upload(ws, [A["last"], A["cur"], B["last"], B["cur"], P["last"], P["cur"], E["last"], E["cur"]])
    jobs = [(A, 0, 1), (B, 2, 3), (E, 6, 7), (P, 4, 5), (A, 0, 1)]
    got = pc.device_ff(ws, sc, jobs=jobs, do_upload=False)
    pc.same_ff(got[3], alone, "pair 3 of 5, an empty pair before it")
    for (Q, _, _), g in zip(jobs, got):
        pc.same_ff(g, pc.oracle_ff(orc, Q, sc["th"], False), "neighbour " + Q["name"])


def test_local_map_result_is_independent_of_slot_and_neighbours(ws, orc):
    sc = pc.lm_scenes()[1]
    by = {F["name"]: F for F in sc["frames"]}
    F, A, B, Z = by["lm_order63"], by["lm_order65"], by["lm_best_3_0.8"], by["lm_zero"]
    alone = pc.device_lm(ws, sc, frames=[F])[0]
    pc.same_lm(alone, pc.oracle_lm(orc, F, sc["th"], sc["nnratio"], sc["cos_limit"]), "frame 0 of 1")
    frames, slots = [A, B, Z, F, A], [5, 1, 2, 6, 5]
    got = pc.device_lm(ws, sc, frames=frames, slots=slots)
    pc.same_lm(got[3], alone, "frame 3 of 5 on slot 6, a frame without points before it")
    for Q, g in zip(frames, got):
        pc.same_lm(g, pc.oracle_lm(orc, Q, sc["th"], sc["nnratio"], sc["cos_limit"]), "neighbour " + Q["name"])
