"""k_pose_optimize and k_pose_edges (csrc/k_pose.h) on the crafted cases of tests/pose_crafted.py, against the CPU oracle
tests/cpp/pose_oracle.cpp and against what each case promises by construction.  test_pose_crafted.py shows on the CPU that the oracle
takes the path each case exists for and that no classified chi2 lies within 1e-6 (relative) of its threshold, so flags and nGood have to
match exactly; the pose within pose_close(..., 1e-5), byte for byte where the problem does not move."""
import ctypes as C

import numpy as np
import pytest

import pose_cases as pc
import pose_crafted as pcr

pytestmark = pytest.mark.gpu

CAM_RING = 8              # SD_SOLVER_RING (csrc/sd_api.hip)


def _pack(names):
    cs = [pcr.cases()[n] for n in names]
    off = np.zeros(len(cs) + 1, np.int32)
    off[1:] = np.cumsum([len(c["edges"]) for c in cs])
    return off, np.concatenate([c["edges"] for c in cs]), [c["cam"] for c in cs], np.stack([c["T0"] for c in cs])


def _run(fe, names):
    """One sd_pose_optimize_host launch of the named cases, each with its own camera -> {name: (Tcw, flags, nGood)}."""
    off, edges, cams, T0 = _pack(names)
    T, out, good = fe.pose_optimize(off, edges, cams, T0)
    return {n: (T[k].copy(), out[off[k]:off[k + 1]].copy(), int(good[k])) for k, n in enumerate(names)}


@pytest.fixture(scope="module")
def batch(gpu, fe):
    return _run(fe, pcr.names())


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def _check_against_oracle(name, got):
    c = pcr.cases()[name]
    T, flags, good = got
    r, To, fo, _, _ = pcr.oracle_result(name)
    assert np.array_equal(flags, fo), (name, np.nonzero(flags != fo)[0][:8])
    assert good == r, name
    assert pc.pose_close(T, To, 1e-5), (name, np.abs(T - To).max())
    if c["no_move"]:
        assert T.tobytes() == To.tobytes() == c["T0"].tobytes(), name
    ex = c["expect"]
    if ex is not None:
        assert np.array_equal(flags, ex["flags"]) and good == ex["n_good"], name
        if "T_bytes" in ex:
            assert T.tobytes() == ex["T_bytes"], name
        if "T_close" in ex:
            assert pc.pose_close(T, ex["T_close"], 1e-5), (name, np.abs(T - ex["T_close"]).max())


@pytest.mark.parametrize("name", pcr.names())
def test_case_matches_oracle_and_expectation(batch, name):
    _check_against_oracle(name, batch[name])


def test_alone_twice_and_reversed_give_the_same_bytes(batch, fe):
    names = pcr.names()
    again = _run(fe, names)
    rev = _run(fe, names[::-1])
    for n in names:
        assert _same(batch[n], again[n]), "two runs differ: " + n
        assert _same(batch[n], rev[n]), "the reversed batch differs: " + n
    for n in names:
        assert _same(batch[n], _run(fe, [n])[n]), "alone differs from batched: " + n


def test_camera_ring_over_many_launches(batch, fe):
    """2 * SD_SOLVER_RING + 1 launches back to back: every table of the ring is reused twice, and regrown when a later launch has
    more problems than the one that last used it.  Successive launches take successive cases, so their cameras differ."""
    names = pcr.names()
    counts = [1, 3, 2, 40, 5, 1, 7, 2, 33, 4, 1, 50, 2, 9, 1, 64, 3]
    assert len(counts) == 2 * CAM_RING + 1
    at = 0
    for k, cnt in enumerate(counts):
        pick = [names[(at + j) % len(names)] for j in range(cnt)]
        pick = list(dict.fromkeys(pick))
        at += cnt
        got = _run(fe, pick)
        for n in pick:
            assert _same(got[n], batch[n]), (k, n)
            _check_against_oracle(n, got[n])


def test_device_entry_on_a_side_stream_equals_the_host_entry(batch, fe):
    import torch
    names = pcr.names()
    off, edges, cams, T0 = _pack(names)
    n = len(names)
    keys = ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")
    cam = np.array([[c.get(k, 0.0) for k in keys] for c in cams], np.float32)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_off = torch.from_numpy(off).cuda(); d_e = torch.from_numpy(edges.view(np.uint8).copy()).cuda()
        d_T = torch.from_numpy(T0.reshape(n, 16).copy()).cuda()
        d_o = torch.full((len(edges),), 0x5A, dtype=torch.uint8, device="cuda"); d_g = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        fe.check(fe.lib().sd_pose_optimize_device(n, C.c_void_p(d_off.data_ptr()), C.c_void_p(d_e.data_ptr()), cam.ctypes.data_as(C.c_void_p),
                                                  C.c_void_p(d_T.data_ptr()), C.c_void_p(d_o.data_ptr()), C.c_void_p(d_g.data_ptr()),
                                                  C.c_void_p(side.cuda_stream)))
        side.synchronize()
        T = d_T.cpu().numpy().reshape(n, 4, 4); out = d_o.cpu().numpy(); good = d_g.cpu().numpy()
    for k, name in enumerate(names):
        assert _same((T[k], out[off[k]:off[k + 1]], int(good[k])), batch[name]), name


def _raw_call(fe, n, off, edges, cams, T, fill=0x5A):
    """sd_pose_optimize_host with sentinel-filled outputs -> (rc, Tcw bytes, outlier, nGood)."""
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    out = np.full(64, fill, np.uint8); good = np.full(max(n, 1), 0x5A5A5A5A, np.int32)
    Tin = None if T is None else T.copy()
    rc = fe.lib().sd_pose_optimize_host(n, p(off), p(edges), p(cams), p(Tin), p(out), p(good))
    return rc, Tin, out, good


def test_invalid_arguments_launch_nothing(gpu, fe):
    c = pcr.cases()["exact_identity_mixed"]
    e = np.ascontiguousarray(c["edges"][:30])
    keys = ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")
    cam = np.array([[c["cam"].get(k, 0.0) for k in keys]] * 2, np.float32)
    T = np.stack([c["T0"], c["T0"]]).reshape(2, 16) + np.float32(0.125)          # not the truth: a launch would change it
    ok = np.array([0, 12, 30], np.int32)
    bad = [("edge_offset[0] != 0", (2, np.array([1, 12, 30], np.int32), e, cam, T)),
           ("a decreasing offset", (2, np.array([0, 20, 12], np.int32), e, cam, T)),
           ("no edge table", (2, ok, None, cam, T)),
           ("no offsets", (2, None, e, cam, T)),
           ("no cameras", (2, ok, e, None, T)),
           ("no poses", (2, ok, e, cam, None)),
           ("a negative problem count", (-1, ok, e, cam, T))]
    for what, args in bad:
        rc, Tout, out, good = _raw_call(fe, *args)
        assert rc == fe.SD_ERR_INVALID, what
        assert (out == 0x5A).all() and (good == 0x5A5A5A5A).all(), what
        assert Tout is None or Tout.tobytes() == T.tobytes(), what
    rc, Tout, out, good = _raw_call(fe, 2, ok, e, cam, T)                          # the same call with valid tables does run
    assert rc == 0 and (out[:30] <= 1).all() and (out[30:] == 0x5A).all() and Tout.tobytes() != T.tobytes()


# ---------------------------------------------------------------- k_pose_edges on uploaded frames
@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    import fuse_cases as fc
    import triangulate_cases as tc
    w = fc.Workspace(fe, 2 * len(pcr.FRAME_SIZES), tc.vocabulary(synth))
    yield w
    w.close()


def _write_matches(fe, ws, rows):
    """Overwrite the match row of projection pair q with rows[q] (the rest of the row -1)."""
    import torch
    d_match, _, _, _, cap = ws.b.matches_device()
    assert cap == ws.cap
    m = fe.as_torch_u8(d_match, len(rows) * cap * 4).view(torch.int32).view(len(rows), cap)
    full = np.full((len(rows), cap), -1, np.int32)
    for q, r in enumerate(rows):
        full[q, :len(r)] = r
    m.copy_(torch.from_numpy(full).cuda())
    torch.cuda.synchronize()


def test_pose_edges_from_a_crafted_match_row(ws, fe):
    import triangulate_cases as tc
    inv = ws.ex.mvInvLevelSigma2
    assert inv.tobytes() == pcr.inv_level_sigma2().tobytes()
    frames = [pcr.edge_frames(N, 900 + k, inv) for k, N in enumerate(pcr.FRAME_SIZES)]
    P = len(frames)
    assert max(pcr.FRAME_SIZES) <= ws.cap
    kfs = [None] * (2 * P)
    for q, f in enumerate(frames):
        kfs[2 * q], kfs[2 * q + 1] = f["last"], f["cur"]
    ws.upload_grid(kfs, tc.CAM)
    for q, f in enumerate(frames):
        ws.b.set_mappoints(2 * q, f["xw"], f["flags"])
    I = np.tile(np.eye(4, dtype=np.float32), (P, 1, 1))
    ws.b.search_by_projection([2 * q + 1 for q in range(P)], [2 * q for q in range(P)], I, I, tc.CAM, 15.0)     # the pairs exist
    ws.b.sync()
    _write_matches(fe, ws, [f["match"] for f in frames])
    prior = np.stack([f["T0"] for f in frames])
    ws.b.pose_optimize(list(range(P)), Tcw=prior)
    for q, f in enumerate(frames):
        N = len(f["match"])
        idx = np.nonzero(f["match"] >= 0)[0]
        Tg, og, ni, ng = ws.b.download_pose(q)
        # the edges k_pose_edges had to build: key-point order, xw[match], mvKeysUn, uRight, invSigma2[octave]
        kp = ws.b.download_keys_un(2 * q + 1)
        xw, _ = ws.b.download_mappoints(2 * q)
        e = np.zeros(len(idx), pc.EDGE_DTYPE)
        e["xw"] = xw[f["match"][idx]]; e["u"] = kp["x"][idx]; e["v"] = kp["y"][idx]; e["ur"] = f["cur"]["ur"][idx]
        e["inv_sigma2"] = inv[kp["octave"][idx]]; e["kp_index"] = idx
        assert e.tobytes() == f["edges"].tobytes(), N
        assert set(kp["octave"][idx]) == set(range(8)) and (e["ur"] < 0).any() and (e["ur"] == 0).any() and (e["ur"] > 0).any()
        r, To, oo, _, rep = pc.optimize_paths(e, f["cam"], f["T0"])
        assert rep["margin"] >= pcr.MARGIN
        assert ni == len(idx), (N, ni)
        assert not og[np.setdiff1d(np.arange(len(og)), idx)].any(), N
        assert np.array_equal(og[idx], oo) and ng == r, (N, np.nonzero(og[idx] != oo)[0][:8])
        assert pc.pose_close(Tg, To, 1e-5), (N, np.abs(Tg - To).max())
        # and the same edges through the plain entry: the same bytes
        Tp, op, gp = fe.pose_optimize(np.array([0, len(e)], np.int32), e, f["cam"], f["T0"][None])
        assert Tp[0].tobytes() == Tg.tobytes() and op.tobytes() == og[idx].tobytes() and gp[0] == ng, N
    # two matches: 0 and the prior untouched; no match: nInitialCorrespondences = 0
    two = np.full(len(frames[0]["match"]), -1, np.int32); two[[64, 200]] = [5, 9]
    _write_matches(fe, ws, [two, np.full(4, -1, np.int32)] + [f["match"] for f in frames[2:]])
    ws.b.pose_optimize([0, 1], Tcw=prior[:2])
    Tg, og, ni, ng = ws.b.download_pose(0)
    assert (ni, ng) == (2, 0) and Tg.tobytes() == prior[0].tobytes() and not og.any()
    Tg, og, ni, ng = ws.b.download_pose(1)
    assert (ni, ng) == (0, 0) and Tg.tobytes() == prior[1].tobytes() and not og.any()
