"""Shared by test_pose_oracle.py and test_gpu_pose.py: the PoseOptimization CPU oracle (tests/cpp/pose_oracle.cpp, compiled with
g++ -O2 -ffp-contract=off into a temporary directory) and seeded synthetic pose problems."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_DTYPE = np.dtype([("xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"), ("kp_index", "<i4")])
CAM = dict(fx=np.float32(718.856), fy=np.float32(718.856), cx=np.float32(607.1928), cy=np.float32(185.2157), mbf=np.float32(386.1448))
MODE_FRESH_ERRORS, MODE_NO_RESTART, MODE_F64_INVZ, MODE_EVAL = 1, 2, 4, 256
MODE_LAMBDA_FMAX, MODE_GEQ, MODE_F64_COMPARE = 8, 16, 32                              # variants, see tests/cpp/pose_oracle.cpp
MODE_FLIP_BRANCH = (128, 512, 1024)                                                     # wrong sign of w in the i = 0 / 1 / 2 branch
QUAT_BRANCHES = ("tr>0", "i=0", "i=1", "i=2")                                            # Quaterniond(Matrix3d)
ROUND_ENDINGS = ("not_run", "ten_iterations", "qmax==10", "rho==0", "nStop>=3", "no_active_edge")

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        d = tempfile.mkdtemp(prefix="pose_oracle_")
        so = os.path.join(d, "libpose_oracle.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "pose_oracle.cpp")])
        L = C.CDLL(so)
        L.sd_pose_oracle.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sd_pose_oracle_paths.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7
        _oracle = L
    return _oracle


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def cam5(cam):
    return np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"]], np.float32)


def optimize(edges, cam, Tcw, mode=0):
    """PoseOptimization on the CPU: (return value, Tcw (4, 4) f32, outlier (E,) u8, stats (13,))."""
    e = np.ascontiguousarray(edges, EDGE_DTYPE)
    T = np.ascontiguousarray(np.array(Tcw, np.float32).reshape(16))
    out = np.full(max(len(e), 1), 7, np.uint8)
    st = np.zeros(13, np.int32)
    r = oracle().sd_pose_oracle(mode, len(e), _p(e), _p(cam5(cam)), _p(T), _p(out), _p(st), None)
    return r, T.reshape(4, 4), out[:len(e)], st


def optimize_paths(edges, cam, Tcw, mode=0):
    """optimize() with the path report: (return value, Tcw, outlier, stats, paths).  paths: quat (the prior's Quaterniond(Matrix3d)
    branch, of QUAT_BRANCHES), w_flip, small_exp (small-angle exp calls), non_finite (some chi2 was inf or NaN), endings (per round run,
    of ROUND_ENDINGS), rejected (trials per round run), reentered (flags that went from outlier to inlier), last_round_changes (flags
    the round without the robust kernel changed), exp_quat (branches the quaternion of an exp took), margin (the smallest
    |chi2 - thr| / thr of any classification)."""
    e = np.ascontiguousarray(edges, EDGE_DTYPE)
    T = np.ascontiguousarray(np.array(Tcw, np.float32).reshape(16))
    out = np.full(max(len(e), 1), 7, np.uint8)
    st = np.zeros(13, np.int32); pa = np.zeros(16, np.int32); mg = np.zeros(1, np.float64)
    r = oracle().sd_pose_oracle_paths(mode, len(e), _p(e), _p(cam5(cam)), _p(T), _p(out), _p(st), _p(pa), _p(mg))
    rounds = int(st[0])
    paths = dict(quat=QUAT_BRANCHES[pa[0]] if pa[0] >= 0 else None, w_flip=bool(pa[1]), small_exp=int(pa[2]), non_finite=bool(pa[3]),
                 endings=[ROUND_ENDINGS[pa[4 + 2 * k]] for k in range(rounds)], rejected=[int(pa[5 + 2 * k]) for k in range(rounds)],
                 reentered=int(pa[12]), last_round_changes=int(pa[13]),
                 exp_quat=[QUAT_BRANCHES[b] for b in range(4) if pa[14] >> b & 1], margin=float(mg[0]))
    return r, T.reshape(4, 4), out[:len(e)], st, paths


def evaluate(edges, cam, q, t, delta, mode=0):
    """Per edge: error at exp(delta) * (q, t) (3,) and the Jacobian at (q, t) (3, 6)."""
    e = np.ascontiguousarray(edges, EDGE_DTYPE)
    aux = np.zeros(13 + 21 * len(e), np.float64)
    aux[0:4] = q; aux[4:7] = t; aux[7:13] = delta
    oracle().sd_pose_oracle(MODE_EVAL | mode, len(e), _p(e), _p(cam5(cam)), None, None, None, _p(aux))
    o = aux[13:].reshape(len(e), 21)
    return o[:, :3].copy(), o[:, 3:].reshape(len(e), 3, 6).copy()


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R; T[:3, 3] = t
    return T


def perturb(T, rng, deg, metres):
    if deg == 0 and metres == 0:
        return T.copy()
    a = rng.normal(size=3); a *= np.deg2rad(deg) / np.linalg.norm(a)
    d = rng.normal(size=3); d *= metres / np.linalg.norm(d)
    return pose(rodrigues(a), d) @ T


def make_problem(rng, n, kind="mixed", outlier_ratio=0.0, noise=0.5, gross=20.0, cam=CAM, T=None):
    """n edges seen from pose T (random when None): points 2 - 40 m in front of the camera, octave 0 - 7, Gaussian pixel noise
    `noise` * scale, an outlier_ratio share moved by >= `gross` px.  Returns (edges, Tcw_true (4, 4) f64, outlier mask)."""
    if T is None:
        T = pose(rodrigues(rng.normal(size=3) * 0.5), rng.normal(size=3) * 2.0)
    fx, fy, cx, cy, bf = [float(cam[k]) for k in ("fx", "fy", "cx", "cy", "mbf")]
    Z = rng.uniform(2.0, 40.0, n)
    u0 = rng.uniform(0, 1241, n); v0 = rng.uniform(0, 376, n)
    Xc = np.stack([(u0 - cx) * Z / fx, (v0 - cy) * Z / fy, Z], 1)
    R, t = T[:3, :3], T[:3, 3]
    Xw = ((Xc - t) @ R).astype(np.float32)                      # R^T (Xc - t)
    Xc = Xw.astype(np.float64) @ R.T + t
    octv = rng.integers(0, 8, n)
    scale = 1.2 ** octv
    e = np.zeros(n, EDGE_DTYPE)
    e["xw"] = Xw
    u = fx * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(size=n) * noise * scale
    v = fy * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(size=n) * noise * scale
    ur = u - bf / Xc[:, 2] + rng.normal(size=n) * noise * scale
    if kind == "mono":
        stereo = np.zeros(n, bool)
    elif kind == "stereo":
        stereo = np.ones(n, bool)
    else:
        stereo = rng.random(n) < 0.6
    bad = rng.random(n) < outlier_ratio
    ang = rng.uniform(0, 2 * np.pi, n); mag = gross + rng.uniform(0, 3 * gross, n)
    u = np.where(bad, u + mag * np.cos(ang), u); v = np.where(bad, v + mag * np.sin(ang), v)
    e["u"] = u; e["v"] = v
    e["ur"] = np.where(stereo & (ur >= 0), ur, -1.0)               # a stereo match needs uR >= 0: the others stay monocular
    e["inv_sigma2"] = (1.0 / (np.float32(1.2) ** (2 * octv)).astype(np.float32)).astype(np.float32)
    e["kp_index"] = np.arange(n)
    return e, T, bad


def pose_close(A, B, tol=1e-5):
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64)
    return (np.max(np.abs(A[:3, :3] - B[:3, :3])) <= tol and
            np.max(np.abs(A[:3, 3] - B[:3, 3])) <= tol * max(1.0, np.linalg.norm(B[:3, 3])))
