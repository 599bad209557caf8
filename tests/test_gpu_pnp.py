"""PnPsolver on the GPU (k_pnp.h through sd_pnp_ransac_host / sd_pnp_ransac_device) against the CPU oracle (tests/cpp/pnp_oracle.cpp) on
the crafted problems of tests/pnp_cases.py: the RANSAC stage byte for byte against the SEQUENTIAL oracle (the counts and poses of every
iteration through the debug download, the best iteration, the best mask and pose), Refine and the final record bit for bit against the
oracle in the kernel's summation order, decisions equal and poses within the recorded spread against the sequential order."""
import json
import os
import subprocess

import numpy as np
import pytest

import pnp_cases as pc

pytestmark = pytest.mark.gpu
TOL_PATH = os.path.join(pc.ROOT, "profiles", "pnp_tolerance.json")


def _groups():
    g = {}
    for pr in pc.ransac_cases():
        g.setdefault(pc.group_key(pr), []).append(pr)
    return g


def _kw(key):
    return dict(zip(("probability", "min_inliers", "max_iterations", "min_set", "epsilon", "th2"), key))


def _f64_differ(a, b):
    """Elementwise: the bits differ, where a NaN equals any NaN (IEEE leaves a NaN's sign and payload open: x86-64 and gfx950 produce
    different ones for 0 / 0; a NaN hypothesis counts no inlier and never reaches a record)."""
    na, nb = np.isnan(a), np.isnan(b)
    return (na != nb) | (~na & (a.view(np.uint64) != b.view(np.uint64)))


@pytest.fixture(scope="module")
def device_results(gpu, fe):
    """{case name: (result, inliers, counts row, poses row)} from one sd_pnp_ransac_host call per argument group, plus the packed calls."""
    by, calls = {}, []
    for key, prs in _groups().items():
        off, corr, probs = pc.pack(prs)
        res, inl, cnt, pos = fe.pnp_ransac(off, corr, probs, counts=True, **_kw(key))
        calls.append((key, prs, off, corr, probs, res, inl))
        for k, pr in enumerate(prs):
            by[pr["name"]] = (res[k], inl[off[k]:off[k + 1]], cnt[k], pos[k])
    return by, calls


@pytest.fixture(scope="module")
def oracle_results():
    return {pr["name"]: (pc.iterate(pr, order=0), pc.iterate(pr, order=1)) for pr in pc.ransac_cases()}


def test_problem_ring_and_workspace_over_many_launches_on_two_streams(gpu, fe):
    """sd_pnp_ransac_device on the schedule of solver_ring.py: every output byte of every call equals the problem run alone through the
    host form.  8 .. 53 correspondences: below and above min_inliers = 10."""
    import ctypes as C
    import torch
    import solver_ring as sr
    pool = [pc.make_problem(300 + k, n, outliers=0.3, noise=0.2, name="ring_%d" % n) for k, n in enumerate(range(8, 56, 3))]
    calls = sr.schedule(pool, lambda pr: len(pr["corr"]))
    D = pc.DEFAULTS
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())

    def prepare(prs):
        off, corr, probs = pc.pack(prs)
        return dict(prs=prs, off=off, probs=probs, corr=torch.from_numpy(corr.view(np.uint8).reshape(-1).copy()).cuda(),
                    res=torch.full((len(prs) * pc.RESULT_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda"),
                    inl=torch.full((len(corr),), 0x5A, dtype=torch.uint8, device="cuda"))

    def enqueue(a, stream):
        fe.check(fe.lib().sd_pnp_ransac_device(len(a["prs"]), p(a["off"]), dp(a["corr"]), p(a["probs"]), D["probability"], D["min_inliers"],
                                               D["max_iterations"], D["min_set"], D["epsilon"], D["th2"], dp(a["res"]), dp(a["inl"]), None, None, 0,
                                               C.c_void_p(stream)))

    done = sr.drive(calls, prepare, enqueue)
    alone = {}
    for k, a in enumerate(done):
        res = a["res"].cpu().numpy().view(pc.RESULT_DTYPE); inl = a["inl"].cpu().numpy(); off = a["off"]
        for q, pr in enumerate(a["prs"]):
            if pr["name"] not in alone:
                alone[pr["name"]] = fe.pnp_ransac(*pc.pack([pr]), **D)
            r, i = alone[pr["name"]]
            assert res[q].tobytes() == r[0].tobytes() and inl[off[q]:off[q + 1]].tobytes() == i.tobytes(), (k, q, pr["name"])


def test_ransac_stage_gives_the_sequential_oracles_bytes(device_results, oracle_results):
    by, _ = device_results
    assert len(by) == len(pc.ransac_cases())
    bad = []
    for pr in pc.ransac_cases():
        name = pr["name"]
        r, inl, cnt, pos = by[name]
        ro, io, _ = oracle_results[name][0]
        end = pc.end_of(pr, ro)
        c, poses, masks = pc.hypotheses(pr, end)
        if cnt[:end].tobytes() != c.tobytes():
            bad.append("%s: %d of %d counts differ" % (name, int((cnt[:end] != c).sum()), end))
        diff = _f64_differ(pos[:end], poses)                         # f64 mRi / mti of every iteration
        if diff.any():
            bad.append("%s: %d of %d hypotheses differ" % (name, int(diff.any(1).sum()), end))
        nan = np.isnan(poses).any(1)                                 # the NaN exemption hides nothing: such a hypothesis counts no inlier, on both sides
        if c[nan].any() or cnt[:end][nan].any():
            bad.append("%s: a NaN hypothesis counts inliers" % name)
        if cnt[end:].any():
            bad.append("%s: counts beyond end" % name)
        for f in ("best_iteration", "best_inliers", "min_inliers", "max_its"):
            if r[f] != ro[f]:
                bad.append("%s.%s: device %d, oracle %d" % (name, f, r[f], ro[f]))
        b = int(ro["best_iteration"])
        if r["kind"] == 2:                                            # the record IS mBestTcw / mvbBestInliers
            T = np.eye(4, dtype=np.float32); T[:3, :3] = poses[b - 1][:9].reshape(3, 3); T[:3, 3] = poses[b - 1][9:]
            if r["Tcw"].tobytes() != T.tobytes() or inl.tobytes() != masks[b - 1].tobytes() or r["n_inliers"] != c[b - 1]:
                bad.append("%s: best pose / mask differ" % name)
    assert not bad, "%d differences, first: %s" % (len(bad), bad[:6])


def test_refine_and_the_record_bit_for_bit_in_the_kernels_order(device_results, oracle_results):
    by, _ = device_results
    bad = []
    for pr in pc.ransac_cases():
        r, inl = by[pr["name"]][:2]
        ro, io, _ = oracle_results[pr["name"]][1]
        for f in pc.RESULT_DTYPE.names:
            if pc.field_bytes(r[f]) != pc.field_bytes(ro[f]):
                bad.append("%s.%s: device %r, oracle %r" % (pr["name"], f, r[f], ro[f]))
        if inl.tobytes() != io.tobytes():
            bad.append("%s: %d inlier bytes differ" % (pr["name"], int(np.sum(inl != io))))
    assert not bad, "%d differences, first: %s" % (len(bad), bad[:6])


def test_against_the_sequential_order(device_results, oracle_results):
    """Decisions equal on every crafted case (each keeps its decision under both orders and both contraction settings -- asserted on the CPU
    by tests/test_pnp_oracle.py and again here, none skipped); poses within 10 x the oracle's own spread for the case, floor 4 f32 ulps."""
    by, _ = device_results
    tol = json.load(open(TOL_PATH))["cases"]
    for pr in pc.ransac_cases():
        name = pr["name"]
        assert pc.stable(pr), name
        r, inl = by[name][:2]
        ro, io, _ = oracle_results[name][0]
        assert (r["kind"], r["iteration"], r["n_inliers"]) == (ro["kind"], ro["iteration"], ro["n_inliers"]) and inl.tobytes() == io.tobytes(), name
        spread = tol[name]["spread"]                              # the recorded figure; tests/test_pnp_oracle.py holds the oracle to it
        fin = np.isfinite(ro["Tcw"])
        assert np.array_equal(fin, np.isfinite(r["Tcw"])), name
        err = np.abs(r["Tcw"][fin].astype(np.float64) - ro["Tcw"][fin])
        bound = np.maximum(10 * spread, 4 * np.spacing(np.abs(ro["Tcw"][fin])).astype(np.float64))
        print("%s: max error %.3g, spread %.3g" % (name, err.max() if len(err) else 0.0, spread))
        assert (err <= bound).all(), (name, float(err.max()), spread)


def test_alone_equals_beside_others_and_reversed(device_results, fe):
    by, calls = device_results
    for name in ("size_65", "outliers_60", "found_at_end", "count_equals_min", "size_%d" % (pc.CHUNK + 1), "resume_new_best", "coincident"):
        pr = next(p for p in pc.ransac_cases() if p["name"] == name)
        res, inl = fe.pnp_ransac(*pc.pack([pr]), **pc.params_of(pr))
        assert pc.same_result(res[0], by[name][0]) and inl.tobytes() == by[name][1].tobytes(), name
    key, prs = max(_groups().items(), key=lambda kv: len(kv[1]))
    off, corr, probs = pc.pack(prs[::-1])
    res, inl = fe.pnp_ransac(off, corr, probs, **_kw(key))
    for k, pr in enumerate(prs[::-1]):
        assert pc.same_result(res[k], by[pr["name"]][0]) and inl[off[k]:off[k + 1]].tobytes() == by[pr["name"]][1].tobytes(), pr["name"]


def test_host_and_device_forms_agree(device_results, fe):
    _, calls = device_results
    for key, prs, off, corr, probs, res, inl in calls:
        r2, i2 = fe.pnp_ransac(off, corr, probs, device=True, **_kw(key))
        assert r2.tobytes() == res.tobytes() and i2.tobytes() == inl.tobytes()          # device against device: NaNs included
        o_res, o_inl = pc.iterate_packed(off, corr, probs, _kw(key), order=1, threads=3)      # the chunked oracle the bench times
        assert all(pc.same_result(res[k], o_res[k]) for k in range(len(prs))) and inl.tobytes() == o_inl.tobytes()


def test_resumed_calls_continue_the_first(device_results, fe):
    by, _ = device_results
    for name in ("resume_same_best", "resume_new_best"):
        pr = next(p for p in pc.ransac_cases() if p["name"] == name)
        first = fe.pnp_ransac(*pc.pack([pr["first_call"]]), **pc.params_of(pr))[0][0]
        assert first["kind"] == 1 and first["iteration"] == pr["prob"]["start_iteration"][0]
        r = by[name][0]
        assert r["kind"] == 1 and r["iteration"] > first["iteration"]
        assert (r["best_iteration"] > first["iteration"]) == (name == "resume_new_best")


def test_invalid_tables_are_refused(gpu, fe):
    pr = pc.make_problem(1, 30)
    off, corr, probs = pc.pack([pr])

    def code(*a, **k):
        with pytest.raises(fe.SdError) as e:
            fe.pnp_ransac(*a, **dict(pc.DEFAULTS, **k))
        return e.value.code

    assert code(off, corr, probs, min_set=3) == fe.SD_ERR_INVALID and code(off, corr, probs, min_set=5) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, max_iterations=0) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, max_iterations=pc.MAX_ITS + 1) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, min_inliers=-1) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, probability=1.0) == fe.SD_ERR_INVALID and code(off, corr, probs, probability=0.0) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, epsilon=0.0) == fe.SD_ERR_INVALID and code(off, corr, probs, epsilon=1.5) == fe.SD_ERR_INVALID
    assert code(off, corr, probs, th2=0.0) == fe.SD_ERR_INVALID and code(off, corr, probs, th2=float("nan")) == fe.SD_ERR_INVALID
    late = probs.copy(); late["start_iteration"] = pc.MAX_ITS - 4
    assert code(off, corr, late) == fe.SD_ERR_INVALID                                                    # start + n_iterations > 4096
    late["start_iteration"] = -1
    assert code(off, corr, late) == fe.SD_ERR_INVALID
    late["start_iteration"] = 0; late["n_iterations"] = 0
    assert code(off, corr, late) == fe.SD_ERR_INVALID
    assert code(off + 1, np.concatenate([corr[:1], corr]), probs) == fe.SD_ERR_INVALID                   # offsets must start at 0
    big = pc.make_problem(1, pc.MAX_N + 1)
    assert code(*pc.pack([big])) == fe.SD_ERR_INVALID                                                    # 4,097: never a truncation
    two = pc.pack([pr, pr])
    dec = two[0].copy(); dec[1], dec[2] = 60, 30
    assert code(dec, two[1], two[2]) == fe.SD_ERR_INVALID                                                # offsets must not decrease
    many = np.zeros(fe.PNP_MAX_PROBLEMS + 1, pc.PROBLEM_DTYPE); many["n_iterations"] = 5                 # a problem is a grid row
    assert code(np.zeros(len(many) + 1, np.int32), corr[:0], many) == fe.SD_ERR_INVALID
    res, inl = fe.pnp_ransac(np.zeros(1, np.int32), corr[:0], probs[:0])                                 # no problem: nothing to do
    assert len(res) == 0 and len(inl) == 0
    last = probs.copy(); last["start_iteration"] = pc.MAX_ITS - 5                                        # the last admissible start
    res, inl = fe.pnp_ransac(off, corr, last, **pc.DEFAULTS)
    ro, io, _ = pc.iterate(dict(pr, prob=last), order=1)
    assert pc.same_result(res[0], ro) and inl.tobytes() == io.tobytes() and res[0]["iteration"] > pc.MAX_ITS - 5


def test_the_mirror_program(gpu, fe, tmp_path):
    """slam-dynamic_amd/host/PnPsolver.h compiled with g++ against the library: iterate(5), then a second call from mnIterations."""
    exe = str(tmp_path / "pnp_mirror")
    lib_dir = os.path.dirname(fe.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(pc.ROOT, "include"), "-I" + os.path.join(pc.ROOT, "slam-dynamic_amd", "host"),
                           os.path.join(pc.ROOT, "tests/cpp/pnp_mirror_main.cpp"), "-o", exe, "-L" + lib_dir, "-lsd_frontend",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "PnPsolver mirror ok" in out.stdout, out.stdout + out.stderr
