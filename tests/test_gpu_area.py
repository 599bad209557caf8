"""GPU parity of the two frame-side window matchers on the crafted frame pair of area_cases.py, byte for byte against the oracle:
k_proj_candidates over windows of 16 / 17 grid columns and 16 / 17 / 64 / 65 hits (distinct and tied distances) and windows cut by
each border; k_local_candidates over windows of 64 / 65 members and one cut at a corner.  test_area_cases.py shows on the CPU that
the pair holds these seams; fuse_cases.py pins the same ones for k_fuse_search."""
import numpy as np
import pytest

import area_cases as ac
import fuse_cases as fc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = fc.Workspace(fe, 2, tc.vocabulary(synth, 5))
    yield w
    w.close()


@pytest.fixture(scope="module")
def sc(ws):
    s = ac.scene()
    ws.upload_grid([s["last"], s["cur"]], ac.CAM)          # slot 0 = the last frame, slot 1 = the current one
    ws.b.set_mappoints(0, s["xw"], s["flags"])
    return s


def test_search_by_projection(ws, sc, orc):
    cur, last = sc["cur"], sc["last"]
    ws.b.search_by_projection([1], [0], ac.IDENTITY[None], ac.IDENTITY[None], ac.CAM, ac.TH_PROJ, False, True)
    m, pairs, nm = ws.b.download_matches(0)
    om, opairs, onm = orc.search_by_projection(cur["kp"], cur["desc"], cur["ur"], last["kp"], last["desc"], sc["xw"], sc["flags"], ac.IDENTITY,
                                               ac.IDENTITY, ac.cam_array(), ws.lv.scale, ac.TH_PROJ, False, True)
    assert nm == onm == len(sc["proj"])
    assert np.array_equal(pairs, opairs), "point pairs"
    assert np.array_equal(m[:len(cur["kp"])], om), "mvpMapPoints assignment"


def test_search_local_map(ws, sc, orc):
    import torch
    cur = sc["cur"]
    pts = np.ascontiguousarray(sc["points"]); M = len(pts)
    d_pts = torch.from_numpy(np.frombuffer(pts.tobytes(), np.uint8).copy()).cuda()
    d_desc = torch.from_numpy(sc["pdesc"].copy()).cuda()
    d_track = torch.zeros(M * orc.TRACK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_pm = torch.zeros(M, dtype=torch.int32, device="cuda")
    d_km = torch.zeros((1, ws.cap), dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws.b.search_local_map([1], np.array([0, M], np.int32), d_pts.data_ptr(), d_desc.data_ptr(), ac.IDENTITY[None], ac.CAM, ac.TH_LOCAL, 0.8,
                          d_track.data_ptr(), d_pm.data_ptr(), d_km.data_ptr(), d_nm.data_ptr())
    ws.b.sync()
    track = d_track.cpu().numpy().view(orc.TRACK_DTYPE); pm = d_pm.cpu().numpy(); km = d_km.cpu().numpy(); nm = d_nm.cpu().numpy()
    otr, opm, okm, onm = orc.search_local_map(cur["kp"], cur["desc"], cur["ur"], pts.view(orc.MAP_POINT_DTYPE), sc["pdesc"], ac.IDENTITY,
                                              ac.cam_array(), ws.lv.scale, ac.TH_LOCAL, 0.8, 0.5)
    assert track.tobytes() == otr.tobytes(), "the isInFrustum records"
    assert nm[0] == onm and onm >= 3
    assert np.array_equal(pm, opm), "per-point matches"
    assert np.array_equal(km[0, :len(cur["kp"])], okm), "F.mvpMapPoints"
