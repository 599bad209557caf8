"""Optimizer::LocalBundleAdjustment on the GPU (k_ba.h through sd_local_ba_host / sd_local_ba_device and frontend.local_bundle_adjustment)
against the CPU oracle on the crafted scenes of ba_cases.py.  Decisions and counts must equal the oracle's exactly; poses, points, normals
and distances within max(10 x the case's recorded spread (profiles/ba_tolerance.json), 4 f32 ulps of the entry): DESIGN Q37."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ba_cases as bc

pytestmark = pytest.mark.gpu
NAMES = list(bc.CASES)
FIELDS = ("Tcw", "xw", "normal", "dist", "level1", "erase")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(bc.ROOT, "profiles", "ba_tolerance.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def together(gpu, fe):
    """Every crafted problem in one launch."""
    return dict(zip(NAMES, fe.local_bundle_adjustment([bc.problem_of(bc.scene(n)) for n in NAMES])))


@pytest.fixture(scope="module")
def alone(gpu, fe):
    return {n: fe.local_bundle_adjustment([bc.problem_of(bc.scene(n))])[0] for n in NAMES}


def same_bits(a, b):
    return all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in FIELDS) and a["stats"].tobytes() == b["stats"].tobytes()


def test_problem_ring_and_workspace_over_many_launches_on_two_streams(gpu, fe):
    """sd_local_ba_device on the schedule of solver_ring.py: every output byte of every call equals the problem run alone through the host
    form, and the Tcw rows of fixed cameras, which no call writes, keep their sentinel."""
    import torch
    import solver_ring as sr
    pool = [bc.problem_of(bc.make_scene(400 + k, 1 + k % 3, 2, 6 + k, stereo_frac=0.6)) for k in range(16)]
    calls = sr.schedule(pool, lambda q: len(q["edges"]))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def prepare(prs):
        ko, nl, po, eo, kfs, xw, ed, ref = fe.pack_ba_problems(prs)
        outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
                for n in (len(kfs) * 64, len(xw) * 12, len(xw) * 12, len(xw) * 4, len(ed), len(ed), len(prs) * 48)]
        return dict(prs=prs, tabs=(ko, nl, po, eo), ins=[dev(kfs), dev(xw), dev(ed), dev(ref)], outs=outs)

    def enqueue(a, stream):
        rc = fe.lib().sd_local_ba_device(len(a["prs"]), *[p(t) for t in a["tabs"]], *[dp(t) for t in a["ins"]], *[dp(o) for o in a["outs"]],
                                         C.c_void_p(stream))
        assert rc == 0, fe.lib().sd_last_error()

    done = sr.drive(calls, prepare, enqueue)
    alone = {}
    for k, a in enumerate(done):
        ko, nl, po, eo = a["tabs"]
        T, xo, nrm, dist, l1, er, st = [o.cpu().numpy() for o in a["outs"]]
        T = T.reshape(-1, 64)
        for q, pr in enumerate(a["prs"]):
            if id(pr) not in alone:
                alone[id(pr)] = fe.local_bundle_adjustment([pr])[0]
            w = alone[id(pr)]
            got = dict(Tcw=T[ko[q]:ko[q] + nl[q]], xw=xo[12 * po[q]:12 * po[q + 1]], normal=nrm[12 * po[q]:12 * po[q + 1]],
                       dist=dist[4 * po[q]:4 * po[q + 1]], level1=l1[eo[q]:eo[q + 1]], erase=er[eo[q]:eo[q + 1]], stats=st[48 * q:48 * q + 48])
            for f in FIELDS + ("stats",):
                assert got[f].tobytes() == w[f].tobytes(), (k, q, f)
            assert (T[ko[q] + nl[q]:ko[q + 1]] == 0x5A).all(), (k, q)


@pytest.mark.parametrize("name", NAMES)
def test_case_matches_oracle(together, recorded, name):
    got, want = together[name], bc.expected(name)
    bad = bc.mismatch(got, want, recorded[name], log=lambda t: print(name, t))
    assert bad is None, bad
    # the final chi2 is a sum of w r^2 with r a difference of pixel coordinates of order 1e2..1e3 that carry ~1e-13 of rounding each
    for rnd in (0, 1):
        assert abs(got["stats"]["chi2"][rnd] - want["stats"]["chi2"][rnd]) <= 1e-9 * max(want["stats"]["chi2"][rnd], 1.0)


def test_one_launch_equals_each_problem_alone(together, alone):
    for n in NAMES:
        assert same_bits(together[n], alone[n]), n


def test_two_runs_are_bit_identical(fe, together):
    again = dict(zip(NAMES, fe.local_bundle_adjustment([bc.problem_of(bc.scene(n)) for n in NAMES])))
    for n in NAMES:
        assert same_bits(together[n], again[n]), n


def raw_call(fe, problems, fill=0x5A):
    """sd_local_ba_host with sentinel-filled outputs; returns (rc, outputs)."""
    ko, nl, po, eo, kfs, xw, ed, ref = fe.pack_ba_problems(problems)
    outs = [np.full(max(len(kfs), 1) * 64, fill, np.uint8), np.full(max(len(xw), 1) * 12, fill, np.uint8), np.full(max(len(xw), 1) * 12, fill, np.uint8),
            np.full(max(len(xw), 1) * 4, fill, np.uint8), np.full(max(len(ed), 1), fill, np.uint8), np.full(max(len(ed), 1), fill, np.uint8),
            np.full(len(problems) * 48, fill, np.uint8)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = fe.lib().sd_local_ba_host(len(problems), p(ko), p(nl), p(po), p(eo), p(kfs), p(xw), p(ed), p(ref), *[p(o) for o in outs])
    return rc, outs


def test_over_cap_and_out_of_range_are_invalid_and_launch_nothing(gpu, fe):
    base = bc.problem_of(bc.scene("small"))

    def grown(n_kf=None, n_local=None, n_pt=None, n_e=None):
        q = dict(base)
        if n_kf is not None:
            q["kfs"] = np.resize(base["kfs"], n_kf); q["n_local"] = n_local
        if n_pt is not None:
            q["xw"] = np.resize(base["xw"], (n_pt, 3)); q["ref_kf"] = np.full(n_pt, -1, np.int32)
        if n_e is not None:
            q["edges"] = np.resize(base["edges"], n_e)
        return q

    def poked(field, value, table="edges", at=3):
        q = dict(base)
        q[table] = base[table].copy()
        if field:
            q[table][field][at] = value
        else:
            q[table][at] = value
        return q

    bad = [grown(n_kf=67, n_local=65), grown(n_kf=130, n_local=1), grown(n_pt=8193),
           grown(n_e=65537), grown(n_kf=3, n_local=4), poked("kf", 3), poked("kf", -1), poked("point", 8), poked("point", -1),
           poked(None, 3, table="ref_kf"), poked(None, -2, table="ref_kf")]
    for q in bad:
        rc, outs = raw_call(fe, [base, q])
        assert rc == -1                                   # SD_ERR_INVALID
        assert all((o == 0x5A).all() for o in outs)
    rc, outs = raw_call(fe, [base, grown(n_kf=64 + 128, n_local=64)])          # at the caps: accepted
    assert rc == 0


def test_device_entry_on_a_stream_equals_the_host_entry(gpu, fe, together):
    import torch
    names = ["mixed", "outliers", "tile_p6", "empty_no_edges"]
    ko, nl, po, eo, kfs, xw, ed, ref = fe.pack_ba_problems([bc.problem_of(bc.scene(n)) for n in names])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_k, d_x, d_e, d_r = dev(kfs), dev(xw), dev(ed), dev(ref)
    outs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (len(kfs) * 64, len(xw) * 12, len(xw) * 12, len(xw) * 4, len(ed), len(ed), len(names) * 48)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())
    rc = fe.lib().sd_local_ba_device(len(names), p(ko), p(nl), p(po), p(eo), dp(d_k), dp(d_x), dp(d_e), dp(d_r), *[dp(o) for o in outs],
                                     C.c_void_p(stream.cuda_stream))
    assert rc == 0, fe.lib().sd_last_error()
    stream.synchronize()
    T, xo, nrm, dist, l1, er, st = [o.cpu().numpy() for o in outs]
    T = T.view(np.float32).reshape(-1, 16); xo = xo.view(np.float32).reshape(-1, 3); nrm = nrm.view(np.float32).reshape(-1, 3)
    dist = dist.view(np.float32); st = st.view(fe.BA_STATS_DTYPE)
    for q, n in enumerate(names):
        got = dict(Tcw=T[ko[q]:ko[q] + nl[q]].reshape(-1, 4, 4), xw=xo[po[q]:po[q + 1]], normal=nrm[po[q]:po[q + 1]], dist=dist[po[q]:po[q + 1]],
                   level1=l1[eo[q]:eo[q + 1]], erase=er[eo[q]:eo[q + 1]], stats=st[q])
        assert same_bits(got, together[n]), n


def test_profiling_changes_nothing_and_reports_every_phase(gpu, fe, together):
    names = ["mixed", "tile_p6", "empty_no_edges"]
    fe.local_ba_profile(len(names), on=True)
    try:
        got = fe.local_bundle_adjustment([bc.problem_of(bc.scene(n)) for n in names])
        ms = fe.local_ba_profile(len(names))
    finally:
        fe.local_ba_profile(len(names), on=False)
    for n, g in zip(names, got):
        assert same_bits(g, together[n]), n
    assert ms.shape == (3, len(fe.BA_PHASES)) and (ms >= 0).all()
    assert (ms[:2, :4] > 0).all() and (ms[:2] < 1000).all()          # lists, linearisation, Schur, factorisation of the two that iterate
    assert (ms[2, 1:] == 0).all()                                      # a no-op problem has its index lists and nothing else
    assert fe.lib().sd_local_ba_profile(len(names) + 1, ms.ctypes.data_as(C.c_void_p)) == -1
