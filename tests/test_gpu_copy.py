"""What "a frame" is, pinned directly: sd_batch_copy_frame / sd_batch_copy_frames move EVERY per-slot array of a slot (the one list
frame_arrays in csrc/sd_api.hip) and touch no other slot.  Everything the ABI can download is compared byte for byte; the two arrays
without a download (the grid's sorted index and cell starts) are covered by a projection search against the copy."""
import numpy as np
import pytest

import stereo_cases as sc

pytestmark = pytest.mark.gpu

GEOM = sc.GEOMS["752x240-8x1.2"]
N_SLOTS = 6                     # three stereo frames: every slot holds results, so every slot can be downloaded before and after
SRC, PAIRS, SAME = 0, [(0, 2), (0, 5)], 3          # destination 2: a left slot (its SAD distances download); 5: an odd slot
# kpCap is a sum of per-level capacities, each a multiple of 8: 420 features -> 480 (every per-slot array starts 16-byte aligned in every
# slot, bar the 4-byte count and the box table), 400 features -> 456 = 8 mod 16 (in an odd slot the flag bytes start 8 bytes off)
ALIGNED, UNALIGNED = 420, 400
DIST = dict(k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628, k3=1.163314)      # the TUM1 lens


def _cfg(n_features, dist):
    cfg = dict(width=GEOM.W, height=GEOM.H, fx=GEOM.fx, fy=GEOM.fx, cx=GEOM.W / 2.0, cy=GEOM.H / 2.0, bf=GEOM.bf, n_features=n_features,
               scale_factor=GEOM.scale_factor, n_levels=GEOM.n_levels, ini_th_fast=20, min_th_fast=7)
    if dist:
        cfg.update(DIST)
    return cfg


def _snap(fe, b, slot):
    """Every download of a slot, as bytes."""
    kp, desc, per_level = b.download(slot)
    ur, dep = b.download_rgbd(slot)
    xw, fl = b.download_mappoints(slot)
    bx = b.download_boxes(slot)
    dkp, ddesc, dur, ddep = b.download_dynamic(slot)
    s = dict(kp=kp, desc=desc, per_level=per_level, uright=ur, depth=dep, grid=b.download_grid(slot), xw=xw, flags=fl,
             keys_un=b.download_keys_un(slot), dyn_kp=dkp, dyn_desc=ddesc, dyn_uright=dur, dyn_depth=ddep, dyn_keys_un=b.download_dynamic_keys_un(slot))
    s.update(("box_" + k, np.asarray(v)) for k, v in bx.items())
    if slot % 2 == 0:
        s["sad"] = b.download_stereo(slot // 2)[2]
    return {k: np.ascontiguousarray(v).tobytes() for k, v in s.items()}


def _scene(fe, synth, n_features, dist):
    cfg = _cfg(n_features, dist)
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], N_SLOTS)
    cam = fe.make_camera(cfg)
    left = list(range(0, N_SLOTS, 2))
    b.extract_host(np.stack([im for t in range(N_SLOTS // 2) for im in synth.stereo_frame(seq=7, t=t, cfg=cfg)[:2]]))
    b.stereo_match(N_SLOTS // 2, cfg["bf"], cfg["fx"])
    if dist:
        b.set_distortion([cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"]], fe.distortion_of(cfg))
        b.undistort(left)
    b.first_separate([SRC], [np.array([[100, 40, 200, 120], [400, 60, 150, 100], [600, 20, 100, 150]], np.float64)], [[1, 2, 3]])
    if dist:
        b.undistort(left)                      # firstSeparate permuted mvKeys: mvKeysUn / mvdynKeysUn follow
    b.assign_grid(N_SLOTS, cam)
    b.unproject(2, N_SLOTS // 2, cam, np.tile(np.eye(4, dtype=np.float32), (N_SLOTS // 2, 1, 1)))
    xw, fl = b.download_mappoints(SRC)
    n = len(b.download(SRC)[0])
    fl = fl[:n].copy()
    fl[::3] |= (fl[::3] > 0).astype(np.uint8) << 1          # Observations() > 0 on a third of the points
    b.set_mappoints(SRC, xw[:n], fl)
    return b, cam


@pytest.mark.parametrize("mode,dist,n_features", [("copy_frame", False, ALIGNED), ("copy_frames", False, ALIGNED), ("copy_frame", True, ALIGNED),
                                                  ("copy_frames", True, ALIGNED), ("copy_frame", False, UNALIGNED), ("copy_frames", True, UNALIGNED)])
def test_every_array_moves_nothing_else_does(gpu, fe, synth, mode, dist, n_features):
    b, cam = _scene(fe, synth, n_features, dist)
    try:
        if n_features == UNALIGNED:
            assert b.cap % 16 != 0 and any(d % 2 for _, d in PAIRS)          # the byte path: flag bytes of an odd slot, 8 bytes off
        else:
            assert b.cap % 16 == 0
        before = [_snap(fe, b, s) for s in range(N_SLOTS)]
        src = before[SRC]
        assert len(src["kp"]) > 28 * 100 and len(src["dyn_kp"]) > 28 * 20 and len(src["box_boxes"]) >= 2 * 32 and len(src["box_boxItems"]) > 4 * 20
        assert np.frombuffer(src["flags"], np.uint8).max() == 3
        if dist:
            assert src["keys_un"] != src["kp"] and src["dyn_keys_un"] != src["dyn_kp"]
        if mode == "copy_frame":
            for s, d in PAIRS:
                b.copy_frame(s, d)
        else:
            b.copy_frames([s for s, _ in PAIRS] + [SAME], [d for _, d in PAIRS] + [SAME])
        after = [_snap(fe, b, s) for s in range(N_SLOTS)]
        moved = {d: s for s, d in PAIRS}
        for slot in range(N_SLOTS):
            want = before[moved.get(slot, slot)]                # a destination equals its source; every other slot (SAME included) is untouched
            for k, v in after[slot].items():
                assert v == want[k], "%s of slot %d after %s" % (k, slot, mode)
        # the copy as mLastFrame (map points, descriptors) and as mCurrentFrame (its grid: the sorted index and the cell starts)
        I = np.eye(4, dtype=np.float32)[None]
        res = []
        for cur, last in ((SRC, SRC), (SRC, PAIRS[1][1]), (PAIRS[0][1], SRC)):
            b.search_by_projection([cur], [last], I, I, cam, 15.0)
            res.append(b.download_matches(0))
        assert res[0][2] > 50
        for m, p, n in res[1:]:
            assert n == res[0][2] and np.array_equal(m, res[0][0]) and np.array_equal(p, res[0][1])
    finally:
        b.close()


def test_copy_frame_refusals(gpu, fe, synth):
    cfg = _cfg(ALIGNED, False)
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], 4)
    try:
        b.extract_host(np.stack(synth.stereo_frame(seq=7, t=0, cfg=cfg)[:2]))
        for s, d in ((1, 1), (2, 0), (0, 4), (0, -1)):          # src == dst, a source slot without results, dst out of range
            with pytest.raises(fe.SdError):
                b.copy_frame(s, d)
        b.copy_frame(0, 3)
        assert b.download(3)[0].tobytes() == b.download(0)[0].tobytes()
    finally:
        b.close()
