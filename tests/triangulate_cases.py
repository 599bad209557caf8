"""Shared by test_triangulate_oracle.py, test_gpu_triangulate.py, tools/fuzz_triangulate.py and tools/bench_triangulate.py: the
CreateNewMapPoints CPU oracle (tests/cpp/triangulate_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary
directory) and seeded crafted keyframes in plain numpy.

A keyframe is (key points with octave and angle, descriptors, uRight, depth, pose); the device tests write it over a workspace
slot's arrays and run sd_batch_compute_bow on it with a small synthetic vocabulary, the CPU side gets the same FeatureVector from
the BoW oracle.  Descriptors are "node prototype plus flipped bits": a feature identity is a level-1 prototype of the vocabulary
with 40 bits flipped (identities of a node are at least 60 bits apart), a candidate for it is the identity with exactly d more bits
flipped, so node membership and every pairwise distance that matters are chosen; check_distances() verifies both.
Seeds depend on the kind of case and its parameters only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
NEW_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("xw", "<f4", (3,))])
TRACE_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("path", "<i4"), ("outcome", "<i4"), ("stereo1", "<i4"),
                        ("stereo2", "<i4"), ("pad", "<i4"), ("cosRays", "<f4"), ("A", "<f4", (16,)), ("x3D", "<f4", (3,))])
BRANCHES = ["shared_node", "skip_mp1", "skip_onlystereo1", "skip_mp2", "skip_onlystereo2", "dist_reject", "dist51", "epipole_excluded",
            "epipole_near_but_stereo", "den_zero", "epi_fail", "epi_pass", "tie_later_wins", "better_failed_worse_passed", "best50",
            "two_idx1_one_idx2", "hist_culled", "big_node", "neigh_skip_stereo", "neigh_skip_mono", "neigh_run"]
PATHS = ["none", "svd", "unproject1", "unproject2"]
OUTCOMES = ["created", "low_parallax", "w0", "z1", "z2", "reproj1_mono", "reproj1_stereo", "reproj2_mono", "reproj2_stereo", "dist0",
            "scale_low", "scale_high", "no_depth"]
REGF = 128                # SD_BOW_REGF: KF2 features of a node that the device's register path holds
LEVELSUP = 2              # on the L = 3 vocabulary: FeatureVector nodes are the level-1 nodes
GEOM = dict(W=640, H=480, nfeatures=600, scale=1.2, nlevels=8)          # the workspace of the crafted cases (its images are never read)
CAM = dict(fx=F32(718.856), fy=F32(718.856), cx=F32(607.1928), cy=F32(185.2157), mbf=F32(386.1448))
CAM["mb"] = F32(CAM["mbf"] / CAM["fx"])
CAM.update(mnMinX=F32(0), mnMaxX=F32(1241), mnMinY=F32(0), mnMaxY=F32(376))


# ---------------------------------------------------------------- the oracle binding
class _KF(C.Structure):
    _fields_ = [("N", C.c_int32), ("nfv", C.c_int32), ("keysUn", C.c_void_p), ("keys", C.c_void_p), ("desc", C.c_void_p), ("uRight", C.c_void_p),
                ("depth", C.c_void_p), ("fvNode", C.c_void_p), ("fvFeat", C.c_void_p), ("hasMp", C.c_void_p), ("Tcw", C.c_void_p)]


class _Cam(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("mb", C.c_float),
                ("scaleFactor", C.c_float), ("nlevels", C.c_int32), ("scale", C.c_void_p), ("sigma2", C.c_void_p)]


_oracles = {}


def oracle(contract="off"):
    """The oracle library; contract = "fast" builds the same source with -ffp-contract=fast (to count the decisions that changes)."""
    if contract not in _oracles:
        d = tempfile.mkdtemp(prefix="triangulate_oracle_")
        so = os.path.join(d, "libtriangulate_oracle.so")
        arch = ["-march=x86-64-v3"] if contract == "fast" else []          # the baseline x86-64 has no FMA to contract into
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=" + contract] + arch + ["-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "triangulate_oracle.cpp")])
        L = C.CDLL(so)
        L.sd_tri_oracle_branches.restype = C.POINTER(C.c_int64)
        L.sd_tri_oracle_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sd_tri_oracle_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.sd_tri_oracle_null4.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.sd_tri_oracle_branch_count() == len(BRANCHES)
        _oracles[contract] = L
    return _oracles[contract]


def host_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def level_tables(scale_factor, nlevels):
    """mvScaleFactor / mvLevelSigma2 as ORBextractor's constructor computes them (ORBextractor.cc:419-430)."""
    s = np.zeros(nlevels, F32); g = np.zeros(nlevels, F32)
    s[0] = 1; g[0] = 1
    for i in range(1, nlevels):
        s[i] = F32(np.float64(s[i - 1]) * np.float64(F32(scale_factor)))
        g[i] = s[i] * s[i]
    return s, g


class Levels:
    def __init__(self, scale_factor=1.2, nlevels=8):
        self.scale_factor, self.nlevels = scale_factor, nlevels
        self.scale, self.sigma2 = level_tables(scale_factor, nlevels)


def _cam_struct(cam, lv):
    c = _Cam(float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam["mbf"]), float(cam["mb"]),
             float(F32(lv.scale_factor)), lv.nlevels, _p(lv.scale).value, _p(lv.sigma2).value)
    return c


def _kf_struct(kf, keep):
    """kf: dict(kp, desc, ur, depth, Tcw, fv (node, feature arrays), has_mp or None, kp_raw or None)"""
    a = dict(kp=np.ascontiguousarray(kf["kp"], KP_DTYPE), desc=np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32),
             ur=np.ascontiguousarray(kf["ur"], F32), depth=np.ascontiguousarray(kf["depth"], F32),
             fn=np.ascontiguousarray(kf["fv"][0], np.uint32), ff=np.ascontiguousarray(kf["fv"][1], np.uint32),
             T=np.ascontiguousarray(kf["Tcw"], F32).reshape(16),
             has=np.ascontiguousarray(kf["has_mp"], np.uint8) if kf.get("has_mp") is not None else None)
    a["raw"] = np.ascontiguousarray(kf["kp_raw"], KP_DTYPE) if kf.get("kp_raw") is not None else a["kp"]
    keep.append(a)
    return _KF(len(a["kp"]), len(a["fn"]), _p(a["kp"]).value, _p(a["raw"]).value, _p(a["desc"]).value, _p(a["ur"]).value, _p(a["depth"]).value,
               _p(a["fn"]).value, _p(a["ff"]).value, _p(a["has"]).value if a["has"] is not None else None, _p(a["T"]).value)


def branches(L, reset=False):
    b = L.sd_tri_oracle_branches()
    out = {name: int(b[i]) for i, name in enumerate(BRANCHES)}
    if reset:
        L.sd_tri_oracle_reset_branches()
    return out


def search(kf1, kf2, cam=CAM, lv=None, only_stereo=False, check_orientation=False, contract="off"):
    """SearchForTriangulation on the CPU -> dict(match (N1,), pairs (n, 2), nmatches, F12 (3, 3), branches)."""
    L = oracle(contract); lv = lv or Levels(); keep = []
    a, b, c = _kf_struct(kf1, keep), _kf_struct(kf2, keep), _cam_struct(cam, lv)
    n1 = len(kf1["kp"])
    match = np.full(max(n1, 1), -1, np.int32); pairs = np.zeros((max(n1, 1), 2), np.int32); npairs = np.zeros(1, np.int32); F = np.zeros(9, F32)
    L.sd_tri_oracle_reset_branches()
    nm = L.sd_tri_oracle_search(C.byref(a), C.byref(b), C.byref(c), int(only_stereo), int(check_orientation), _p(match), _p(pairs), _p(npairs), _p(F))
    return dict(match=match[:n1].copy(), pairs=pairs[:npairs[0]].copy(), nmatches=nm, F12=F.reshape(3, 3), branches=branches(L))


def create(kf1, neighbours, median_depth=None, cam=CAM, lv=None, contract="off"):
    """CreateNewMapPoints on the CPU -> dict(new (NEW_DTYPE), trace (TRACE_DTYPE, one record per triangulated match), branches)."""
    L = oracle(contract); lv = lv or Levels(); keep = []
    a, c = _kf_struct(kf1, keep), _cam_struct(cam, lv)
    arr = (_KF * max(len(neighbours), 1))(*[_kf_struct(k, keep) for k in neighbours])
    n1 = len(kf1["kp"])
    md = np.ascontiguousarray(median_depth, F32) if median_depth is not None else None
    out = np.zeros(max(n1, 1), NEW_DTYPE); cap = max(1, n1 * max(1, len(neighbours))); tr = np.zeros(cap, TRACE_DTYPE); nt = np.zeros(1, np.int32)
    L.sd_tri_oracle_reset_branches()
    n = L.sd_tri_oracle_create(C.byref(a), len(neighbours), arr, _p(md), C.byref(c), _p(out), _p(tr), cap, _p(nt))
    return dict(new=out[:n].copy(), trace=tr[:nt[0]].copy(), branches=branches(L))


def null4(A, sweeps=None, contract="off"):
    """The frozen null vector of a 4x4 f32 matrix -> (x f32 (4,), the same before narrowing f64 (4,))."""
    L = oracle(contract)
    if sweeps is not None:
        L.sd_tri_oracle_set_sweeps(int(sweeps))
    A = np.ascontiguousarray(A, F32).reshape(16); x = np.zeros(4, F32); v = np.zeros(4, np.float64)
    L.sd_tri_oracle_null4(_p(A), _p(x), _p(v))
    if sweeps is not None:
        L.sd_tri_oracle_set_sweeps(8)
    return x, v


def first_surviving(per_neighbour):
    """The device's formulation in numpy: per_neighbour[k] = records (idx1, idx2, xw) that survive when neighbour k is run ALONE
    against the keyframe's initial map points, ascending idx1.  -> NEW_DTYPE records: the first surviving neighbour per idx1."""
    taken, out = set(), []
    for k, recs in enumerate(per_neighbour):
        for r in recs:
            if int(r["idx1"]) not in taken:
                taken.add(int(r["idx1"]))
                out.append((k, int(r["idx1"]), int(r["idx2"]), r["xw"]))
    return np.array(out, NEW_DTYPE) if out else np.zeros(0, NEW_DTYPE)


# ---------------------------------------------------------------- geometry
def rodrigues(w):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


T1_DEFAULT = pose(rodrigues([0.02, -0.03, 0.01]), [0.3, -0.2, 0.5])


def neighbour_pose(T1, centre_in_cam1, rotvec=(0.0, 0.0, 0.0)):
    """Tcw of a camera whose centre is `centre_in_cam1` (KF1's camera frame) and whose axes are KF1's turned by rotvec."""
    R = rodrigues(rotvec)
    return pose(R, -R @ np.asarray(centre_in_cam1, np.float64)) @ T1


def project(T, Xw, cam=CAM):
    """Projective image of world points: (u, v, z); z may be negative (the image point still lies on the epipolar line)."""
    Xc = np.atleast_2d(Xw) @ T[:3, :3].T + T[:3, 3]
    return float(cam["fx"]) * Xc[:, 0] / Xc[:, 2] + float(cam["cx"]), float(cam["fy"]) * Xc[:, 1] / Xc[:, 2] + float(cam["cy"]), Xc[:, 2]


def to_world(T, Xc):
    return (np.atleast_2d(Xc) - T[:3, 3]) @ T[:3, :3]


# ---------------------------------------------------------------- descriptors
def vocabulary(synth, seed=5):
    """The small synthetic vocabulary test_gpu_bow.py uses (k = 10, L = 3), every word weighted: no feature drops out of a FeatureVector."""
    voc = synth.vocabulary(k=10, L=3, seed=seed, early_leaf_frac=0.0, stop_frac=0.0)
    return voc


def prototypes(voc):
    """(node id, descriptor) of the level-1 nodes: the FeatureVector nodes at LEVELSUP."""
    first = np.nonzero(voc["parent"] == 0)[0]
    return first + 1, voc["desc"][first]


def _flip(desc, bits):
    d = desc.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class Descriptors:
    """Identities and candidates of one vocabulary.  identity(node_slot, k): the k-th identity of level-1 node `node_slot`."""

    def __init__(self, voc, seed):
        self.ids, self.protos = prototypes(voc)
        self.rng = np.random.default_rng(1000 + seed)
        self.pool = {}

    def identity(self, slot, k):
        pool = self.pool.setdefault(slot, [])
        while len(pool) <= k:
            for _ in range(10000):
                d = _flip(self.protos[slot], self.rng.choice(256, 40, replace=False))
                if not pool or np.unpackbits(np.array(pool) ^ d, axis=1).sum(1).min() >= 60:
                    pool.append(d)
                    break
            else:
                raise AssertionError("no room for another identity in node %d" % slot)
        return pool[k]

    def candidate(self, ident, d):
        """`ident` with exactly d bits flipped."""
        return _flip(ident, self.rng.choice(256, d, replace=False))


class KeyFrameBuilder:
    def __init__(self, Tcw):
        self.Tcw = np.asarray(Tcw, np.float64)
        self.rows, self.desc, self.ur, self.depth, self.has, self.raw = [], [], [], [], [], []

    def add(self, u, v, desc, octave=0, angle=0.0, stereo_z=None, ur=None, depth=None, has_mp=False, cam=CAM, raw=None):
        """stereo_z: the feature is a stereo point of that depth (uRight = u - mbf / z); ur / depth override it.  (u, v) is mvKeysUn;
        raw = the mvKeys position where it differs (a distorted camera)."""
        k = np.zeros((), KP_DTYPE)
        k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = u, v, 31.0, angle, 50.0, octave, -1
        r = k.copy()
        if raw is not None:
            r["x"], r["y"] = raw
        self.raw.append(r)
        self.rows.append(k); self.desc.append(np.asarray(desc, np.uint8))
        z = F32(stereo_z) if stereo_z is not None else F32(-1)
        self.depth.append(F32(depth) if depth is not None else z)
        self.ur.append(F32(ur) if ur is not None else (F32(F32(u) - cam["mbf"] / z) if stereo_z is not None else F32(-1)))
        self.has.append(1 if has_mp else 0)
        return len(self.rows) - 1

    def build(self):
        n = len(self.rows)
        return dict(kp=np.array(self.rows, KP_DTYPE) if n else np.zeros(0, KP_DTYPE), desc=np.array(self.desc, np.uint8).reshape(n, 32),
                    ur=np.array(self.ur, F32), depth=np.array(self.depth, F32), Tcw=self.Tcw.astype(F32),
                    has_mp=np.array(self.has, np.uint8) if any(self.has) else None,
                    kp_raw=np.array(self.raw, KP_DTYPE) if any(a != b for a, b in zip(self.raw, self.rows)) else None)


def attach_bow(kfs, voc_oracle, levelsup=LEVELSUP):
    """The FeatureVector of every keyframe from the BoW oracle (CPU tests; the device tests compare against the same)."""
    for k in kfs:
        bow = voc_oracle.compute_bow(k["desc"], levelsup) if len(k["desc"]) else dict(fv_node=np.zeros(0, np.uint32), fv_feature=np.zeros(0, np.uint32))
        k["fv"] = (bow["fv_node"], bow["fv_feature"])
    return kfs


def check_distances(kf1, kf2, want):
    """Node membership and distances are the chosen ones: want = {(i1, i2): d}; every other pair of one node is more than 55 apart."""
    node1 = dict(zip(kf1["fv"][1].tolist(), kf1["fv"][0].tolist())); node2 = dict(zip(kf2["fv"][1].tolist(), kf2["fv"][0].tolist()))
    assert len(node1) == len(kf1["kp"]) and len(node2) == len(kf2["kp"]), "a feature dropped out of its FeatureVector"
    if not len(kf1["kp"]) or not len(kf2["kp"]):
        return
    D = np.unpackbits(kf1["desc"][:, None, :] ^ kf2["desc"][None, :, :], axis=2).sum(2)
    for (i1, i2), d in want.items():
        assert node1[i1] == node2[i2], "features %d / %d were meant to share a node" % (i1, i2)
        assert D[i1, i2] == d, "distance %d / %d is %d, meant %d" % (i1, i2, D[i1, i2], d)
    for i1 in range(len(kf1["kp"])):
        for i2 in range(len(kf2["kp"])):
            if (i1, i2) not in want and node1[i1] == node2[i2]:
                assert D[i1, i2] > 55, "unplanned close pair %d / %d: %d" % (i1, i2, D[i1, i2])


# ---------------------------------------------------------------- crafted cases
# A case: dict(name, kf1, neighbours [kf], median_depth or None, want [per neighbour {(i1, i2): d}], only_stereo, check_orientation,
# expect: branch / outcome names it was built to reach).  Matcher cases have one neighbour and run through search(); the others
# through create().
LATERAL = (1.0, 0.1, 0.3)            # centre of the usual neighbour in KF1's camera frame: 1 m sideways
FORWARD = (0.1, 0.0, 0.8)            # mostly along the optical axis: little ray parallax near the axis


def _pt(T1, x, y, z):
    return to_world(T1, [x, y, z])[0]


def matcher_case(name, D, T1=T1_DEFAULT):
    """Every matcher branch in one pair (except those that need a call of their own, see matcher_cases)."""
    T2 = neighbour_pose(T1, LATERAL, (0.0, 0.02, 0.0))
    A, B = KeyFrameBuilder(T1), KeyFrameBuilder(T2)
    want, notes = {}, {}
    k = [0]

    def ident(slot=0):
        k[0] += 1
        return D.identity(slot, k[0] - 1)

    def both(X, slot=0, d=10, st1=False, st2=False, oct1=0, oct2=0, off2=(0.0, 0.0), ang1=0.0, ang2=0.0, has1=False, has2=False, idn=None):
        idn = ident(slot) if idn is None else idn
        u1, v1, z1 = project(T1, X); u2, v2, z2 = project(T2, X)
        i1 = A.add(u1[0], v1[0], idn, oct1, ang1, stereo_z=z1[0] if st1 else None, has_mp=has1)
        i2 = B.add(u2[0] + off2[0], v2[0] + off2[1], D.candidate(idn, d), oct2, ang2, stereo_z=z2[0] if st2 else None, has_mp=has2)
        want[(i1, i2)] = d
        return i1, i2, idn

    # plain matches, mono / stereo mixes, two nodes
    notes["plain"] = [both(_pt(T1, -2 + j, 0.5 * j, 8 + 2 * j), slot=j % 2, d=5 * j, st1=j % 2 == 1, st2=j % 3 == 1)[:2] for j in range(6)]
    # dist 50 accepted, 51 rejected
    notes["d50"] = both(_pt(T1, 1.5, -1, 9), d=50)[:2]
    notes["d51"] = both(_pt(T1, 2.5, -1, 9), d=51)[:2]
    # a tie at distance 20: the later feature of KF2 wins
    X = _pt(T1, -3, 1, 12)
    i1, i2a, idn = both(X, d=20)
    u, v, _ = project(T2, _pt(T1, -3 * 14 / 12, 14 / 12, 14))          # the same ray of KF1, further out: still on the epipolar line
    i2b = B.add(u[0], v[0], D.candidate(idn, 20)); want[(i1, i2b)] = 20
    notes["tie"] = (i1, i2a, i2b)
    # the better candidate (d = 8) is 30 px off the epipolar line, the worse (d = 30) is on it; once in each order
    for order in (0, 1):
        X = _pt(T1, 3 + order, 1.5, 11)
        idn = ident(0)
        u1, v1, _ = project(T1, X); u2, v2, _ = project(T2, X)
        i1 = A.add(u1[0], v1[0], idn)
        cands = [(D.candidate(idn, 8), u2[0], v2[0] + 30.0, 8), (D.candidate(idn, 30), u2[0], v2[0], 30)]
        if order:
            cands.reverse()
        ii = [B.add(cu, cv, cd) for (cd, cu, cv, _) in cands]
        for j, c in zip(ii, cands):
            want[(i1, j)] = c[3]
        notes["better_fails_%d" % order] = (i1, ii[0 if order else 1])
    # the epipole exclusion: a KF2 feature half a pixel from the epipole lies on every epipolar line; excluded for mono-mono only
    Ow1 = to_world(T1, [0.0, 0.0, 0.0])[0]
    ex, ey, _ = project(T2, Ow1)
    for st1 in (False, True):
        idn = ident(1)
        i1 = A.add(300.0 + 50 * st1, 120.0, idn, stereo_z=9.0 if st1 else None)
        i2 = B.add(ex[0] + 0.5, ey[0], D.candidate(idn, 12)); want[(i1, i2)] = 12
        notes["epipole_stereo1" if st1 else "epipole_mono"] = (i1, i2)
    # has_mp1: skipped although its candidate is perfect; has_mp2: the best candidate is taken, the second wins
    notes["has_mp1"] = both(_pt(T1, -1, -1.5, 7), d=3, has1=True)[:2]
    X = _pt(T1, 0.5, 2, 10)
    i1, i2a, idn = both(X, d=4, has2=True)
    u, v, _ = project(T2, X)
    i2b = B.add(u[0], v[0], D.candidate(idn, 25)); want[(i1, i2b)] = 25
    notes["has_mp2"] = (i1, i2a, i2b)
    # two features of KF1 take one feature of KF2
    X = _pt(T1, -0.5, 0.3, 6)
    i1a, i2, idn = both(X, d=6)
    u1, v1, _ = project(T1, X)
    near = D.candidate(idn, 2)
    i1b = A.add(u1[0], v1[0], near); want[(i1b, i2)] = hamming(near, B.desc[i2])
    notes["shared_idx2"] = (i1a, i1b, i2)
    # rotation histogram: the matches turn by 0 degrees, one by 90: less than a tenth of the top bin, culled when the histogram is on
    notes["rot90"] = [both(_pt(T1, 4, -2, 15), slot=1, d=7, ang1=100.0, ang2=10.0)[:2]]
    # a node of KF2 with more features than the register path holds: REGF + 1 in node slot 2, the candidate the last of them
    X = _pt(T1, -4, -1, 20)
    idn = ident(2)
    u1, v1, _ = project(T1, X); u2, v2, _ = project(T2, X)
    i1 = A.add(u1[0], v1[0], idn)
    for j in range(REGF):
        B.add(u2[0], v2[0], ident(2))                                     # fillers: on the line, 60+ bits away
    i2 = B.add(u2[0], v2[0], D.candidate(idn, 9)); want[(i1, i2)] = 9
    notes["big_node"] = (i1, i2)
    # a node only KF1 has, a node only KF2 has
    A.add(100.0, 100.0, ident(3)); B.add(100.0, 100.0, ident(4))
    return dict(name=name, kf1=A.build(), neighbours=[B.build()], median_depth=None, want=[want], notes=notes)


def matcher_cases(synth, seed=5):
    """-> (voc, [case]): `all` (every branch one pair can hold), `identical_poses` (F12 = 0: den == 0), `empty1` / `empty2` (N = 0),
    `single` (N = 1 on both sides), `no_shared_node`."""
    voc = vocabulary(synth, seed)
    D = Descriptors(voc, seed)
    cases = [matcher_case("all", D)]
    c = matcher_case("identical_poses", Descriptors(voc, seed), pose(np.eye(3), [0.3, -0.2, 0.5]))     # no rotation: R12 = I and t12 = 0 exactly
    c["neighbours"][0]["Tcw"] = c["kf1"]["Tcw"].copy()
    cases.append(c)
    T2 = neighbour_pose(T1_DEFAULT, LATERAL)
    X = _pt(T1_DEFAULT, 0.4, 0.2, 9)
    for name in ("empty1", "empty2", "single", "no_shared_node"):
        A, B = KeyFrameBuilder(T1_DEFAULT), KeyFrameBuilder(T2)
        idn = D.identity(5, 0)
        u1, v1, _ = project(T1_DEFAULT, X); u2, v2, _ = project(T2, X)
        want = {}
        if name != "empty1":
            A.add(u1[0], v1[0], idn)
        if name != "empty2":
            B.add(u2[0], v2[0], D.candidate(idn, 11) if name != "no_shared_node" else D.identity(6, 0))
        if name == "single":
            want[(0, 0)] = 11
        cases.append(dict(name=name, kf1=A.build(), neighbours=[B.build()], median_depth=None, want=[want], notes={}))
    return voc, cases


def triangulation_case(D, T1=T1_DEFAULT):
    """One keyframe, four neighbours, one feature per triangulation branch.  notes[name] = (neighbour, idx1)."""
    Ts = [neighbour_pose(T1, LATERAL, (0.0, 0.02, 0.0)), neighbour_pose(T1, FORWARD, (0.0, 0.0, 0.01)),
          neighbour_pose(T1, (0.2, 0.0, 5.0)), neighbour_pose(T1, (0.6, 0.0, 0.2), (0.0, np.pi, 0.0))]
    A = KeyFrameBuilder(T1); Bs = [KeyFrameBuilder(T) for T in Ts]
    wants = [{} for _ in Ts]; notes = {}
    k = [0]

    def feat(name, nb, X, st1=False, st2=False, oct1=0, oct2=0, d=10, slot=0, off2=(0.0, 0.0), depth1=None, depth2=None, ur1=None, ur2=None,
             flip_disparity=False):
        idn = D.identity(slot, k[0]); k[0] += 1
        u1, v1, z1 = project(T1, X); u2, v2, z2 = project(Ts[nb], X)
        if flip_disparity:                                # mirror kp2 about kp1's own image in KF2 at infinity: the rays diverge
            far = to_world(T1, (np.atleast_2d(X) @ T1[:3, :3].T + T1[:3, 3]) * 1e6)[0]
            uf, vf, _ = project(Ts[nb], far)
            u2, v2 = 2 * uf - u2, 2 * vf - v2
        i1 = A.add(u1[0], v1[0], idn, oct1, stereo_z=(depth1 if depth1 is not None else z1[0]) if st1 else None, ur=ur1)
        i2 = Bs[nb].add(u2[0] + off2[0], v2[0] + off2[1], D.candidate(idn, d), oct2, stereo_z=(depth2 if depth2 is not None else z2[0]) if st2 else None, ur=ur2)
        wants[nb][(i1, i2)] = d
        notes[name] = (nb, i1)
        return i1, i2

    P = lambda x, y, z: _pt(T1, x, y, z)
    # neighbour 0, 1 m sideways: about 5.7 degrees of parallax at 10 m
    feat("svd_mono_mono", 0, P(0.5, 0.2, 10))
    feat("svd_stereo_mono", 0, P(-1.5, 0.4, 9), st1=True)
    feat("svd_mono_stereo", 0, P(1.5, -0.4, 11), st2=True)
    feat("svd_both_stereo", 0, P(2.0, 0.8, 8), st1=True, st2=True)
    feat("mono_mono_parallel", 0, P(3.0, 1.0, 400))                                    # cos >= 0.9998 and no stereo: skipped
    feat("z1_negative", 0, P(-2.5, -0.5, 10), flip_disparity=True)
    feat("reproj1_mono", 0, P(0.2, -1.2, 10), oct1=0, oct2=7, off2=(0.0, 6.0))        # 6 px off the line passes level 7's bound in KF2, not level 0's in KF1
    feat("reproj1_stereo", 0, P(-0.8, 1.1, 10), st1=True, depth1=8.0)                   # uRight says 8 m, the rays say 10 m
    feat("created_off_line", 0, P(0.9, 1.3, 10), oct1=1, oct2=0, off2=(0.0, 1.5))     # 1.5 px off the line: inside every bound
    feat("reproj2_stereo_svd", 0, P(-3.0, 1.4, 10), st2=True, depth2=8.0)
    feat("scale_low", 0, P(1.1, -1.0, 10), oct1=7, oct2=0)
    feat("scale_high", 0, P(-1.1, -1.3, 10), oct1=0, oct2=7)
    # neighbour 1, 0.8 m forward: a point near the axis at 20 m has less ray parallax than its own stereo baseline
    feat("unproject1", 1, P(0.4, 0.1, 20), st1=True)
    feat("unproject2", 1, P(-0.4, 0.2, 20), st2=True)
    feat("quirk_both_stereo", 1, P(0.3, -0.2, 20), st1=True, st2=True)                # cosParallaxStereo2 stays cos + 1: unprojected from KF1
    feat("reproj2_mono", 1, P(0.6, 0.3, 20), st1=True, depth1=6.0)                      # KF1's depth is wrong: its point lands elsewhere on KF2's line
    feat("reproj2_stereo", 1, P(-0.6, -0.3, 20), st1=True, st2=True, depth1=6.0)
    feat("reproj1_mono_unproject2", 1, P(0.2, 0.4, 20), st2=True, depth2=6.0)
    feat("no_depth", 1, P(0.5, -0.1, 20), st1=True, depth1=-1.0)                         # uRight >= 0 but no depth: UnprojectStereo gives no point
    # neighbour 2, 5 m ahead: a point 3 m in front of KF1 is behind it
    feat("z2_negative", 2, P(0.5, 0.0, 3))
    # neighbour 3 looks backwards: the rays of a point in front of KF1 are opposed
    feat("cos_negative", 3, P(0.3, 0.1, 10))
    # the neighbour loop: created with neighbour 0, so absent at neighbour 1; rejected at neighbour 0 (behind), created at neighbour 1
    X = P(-0.2, 0.6, 12)
    i1, _ = feat("created_then_absent", 0, X)
    u, v, _ = project(Ts[1], X)
    wants[1][(i1, Bs[1].add(u[0], v[0], D.candidate(A.desc[i1], 10)))] = 10
    X = P(2.2, -0.7, 9)
    i1, _ = feat("rejected_then_created", 0, X, flip_disparity=True)
    u, v, z = project(Ts[1], X)
    wants[1][(i1, Bs[1].add(u[0], v[0], D.candidate(A.desc[i1], 10), stereo_z=z[0]))] = 10
    return dict(name="branches", kf1=A.build(), neighbours=[B.build() for B in Bs], median_depth=None, want=wants, notes=notes)


def neighbour_cases(D, T1=T1_DEFAULT):
    """zero neighbours; a neighbour skipped by the stereo rule (baseline < mb); one skipped by the monocular rule (baseline / median < 0.01)."""
    out = []
    X = _pt(T1, 0.5, 0.2, 10)
    for name, centres, median in (("zero_neighbours", [], None), ("stereo_rule", [(0.3, 0.0, 0.0), LATERAL], None),
                                  ("mono_rule", [LATERAL, (1.0, 0.0, 0.0)], [200.0, 20.0])):
        A = KeyFrameBuilder(T1); idn = D.identity(7, len(out))
        u1, v1, _ = project(T1, X)
        A.add(u1[0], v1[0], idn)
        Bs, wants = [], []
        for c in centres:
            T2 = neighbour_pose(T1, c)
            B = KeyFrameBuilder(T2)
            u2, v2, _ = project(T2, X)
            B.add(u2[0], v2[0], D.candidate(idn, 10))
            Bs.append(B.build()); wants.append({(0, 0): 10})
        out.append(dict(name=name, kf1=A.build(), neighbours=Bs, median_depth=median, want=wants, notes={}))
    return out


def nonrigid_case(D):
    """`x3D[3] == 0` (LocalMapping.cc:334).  No rigid pair of poses reaches it, but the call takes any 4x4: with Rcw = diag(0, 1, 1) in
    both poses the first column of A is exactly zero, the Jacobi never turns it, its norm 0 is the smallest, the null vector is e0."""
    R = np.diag([0.0, 1.0, 1.0])
    T1, T2 = pose(R, [0.0, 0.0, 0.0]), pose(R, [0.0, 1.0, 0.2])
    fx, fy, cx, cy = [float(CAM[k]) for k in ("fx", "fy", "cx", "cy")]
    Ki = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])
    t12 = -R @ R.T @ T2[:3, 3] + T1[:3, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = Ki.T @ tx @ (R @ R.T) @ Ki
    A, B = KeyFrameBuilder(T1), KeyFrameBuilder(T2)
    want = {}
    for j, (u1, v1, u2) in enumerate([(cx + 50.0, cy, cx - 80.0), (cx - 120.0, cy + 30.0, cx + 200.0)]):
        a, b, c = F12.T @ np.array([u1, v1, 1.0])                      # the epipolar line of kp1 in KF2: a row (a == 0, x does not matter)
        assert a == 0 and abs(b) > 1e-12
        idn = D.identity(8, j)
        i1 = A.add(u1, v1, idn)
        i2 = B.add(u2, -c / b, D.candidate(idn, 10))
        want[(i1, i2)] = 10
    return dict(name="nonrigid_w0", kf1=A.build(), neighbours=[B.build()], median_depth=None, want=[want], notes={})


def raw_keys_case(D, T1=T1_DEFAULT):
    """UnprojectStereo reads mvKeys, not mvKeysUn (KeyFrame.cc:620-621): stereo points whose raw position lies 1.5 px from the undistorted
    one, unprojected from KF1 (feature 0) and from KF2 (feature 1).  notes[name] = (idx1, camera pose, raw (u, v), depth)."""
    T2 = neighbour_pose(T1, FORWARD, (0.0, 0.0, 0.01))
    A, B = KeyFrameBuilder(T1), KeyFrameBuilder(T2)
    want, notes = {}, {}
    for j, (name, X) in enumerate((("unproject1", _pt(T1, 0.4, 0.1, 20)), ("unproject2", _pt(T1, -0.4, 0.2, 20)))):
        idn = D.identity(9, j)
        u1, v1, z1 = project(T1, X); u2, v2, z2 = project(T2, X)
        st1 = name == "unproject1"
        i1 = A.add(u1[0], v1[0], idn, stereo_z=z1[0] if st1 else None, raw=(u1[0] + 1.5, v1[0] - 0.5) if st1 else None)
        i2 = B.add(u2[0], v2[0], D.candidate(idn, 10), stereo_z=None if st1 else z2[0], raw=None if st1 else (u2[0] - 1.5, v2[0] + 0.5))
        want[(i1, i2)] = 10
        notes[name] = (i1, T1 if st1 else T2, (u1[0] + 1.5, v1[0] - 0.5) if st1 else (u2[0] - 1.5, v2[0] + 0.5), float(F32(z1[0] if st1 else z2[0])))
    return dict(name="raw_keys", kf1=A.build(), neighbours=[B.build()], median_depth=None, want=[want], notes=notes)


def creation_cases(synth, seed=6):
    """-> (voc, cases).  `raw_keys` has key points that differ from their undistorted ones: it runs on the CPU, and on the device only in
    a workspace with a distortion (which computes mvKeysUn itself)."""
    voc = vocabulary(synth, seed)
    D = Descriptors(voc, seed)
    return voc, [triangulation_case(D)] + neighbour_cases(D) + [nonrigid_case(D), raw_keys_case(D)]


SCAN_KINDS = ("epipolar", "reproj1_mono", "reproj1_stereo", "reproj2_mono", "reproj2_stereo")


SCAN_WINDOWS = 16         # geometries per scan, each with its own crossing
SCAN_FORWARD = (0.0, -0.1, 0.6)      # a neighbour ahead whose ray parallax stays below the stereo parallax out to the image border


def from_pixel(T, u, v, z, cam=CAM):
    """The world point that camera T sees at pixel (u, v) and depth z."""
    return to_world(T, [(u - float(cam["cx"])) / float(cam["fx"]) * z, (v - float(cam["cy"])) / float(cam["fy"]) * z, z])[0]


def _scan_rows(kind, items, D, T1=T1_DEFAULT):
    """One (kp1, kp2) pair per item (geometry variant, sliding value); feature j of both keyframes belongs to items[j].  What slides:
    epipolar        kp2.y across the epipolar line (nearly horizontal), both at level 0: CheckDistEpipolarLine's 3.84 sigma^2
    reproj1_stereo  uRight of kp1, reproj2_stereo uRight of kp2: the 7.8 sigma^2 of that camera
    reproj2_mono    kp2.y ALONG the epipolar line of a neighbour 0.6 m ahead (the line is the column of the epipole), the point
                    unprojected from KF1's stereo depth: KF2's 5.991 sigma^2
    reproj1_mono    kp2.y as in reproj2_mono, but kp2 is the stereo point and is unprojected: KF1's 5.991 sigma^2
    The geometries put the sliding coordinate within a few pixels of 0, where one f32 step moves the squared error by about one of
    ITS ulps: at 600 px a step would move it by hundreds, and a contraction (which moves it by one) would hardly ever flip a decision.
    -> (kf1, kf2, per item the value at which the pair is consistent)"""
    forward = kind in ("reproj1_mono", "reproj2_mono")
    T2 = neighbour_pose(T1, SCAN_FORWARD) if forward else neighbour_pose(T1, LATERAL, (0.0, 0.02, 0.0))
    A, B = KeyFrameBuilder(T1), KeyFrameBuilder(T2)
    good = []
    for j, (variant, val) in enumerate(items):
        small = 0.05 + 0.11 * variant                     # where the sliding coordinate is consistent
        z = 10.0 + 0.9 * variant
        mbf = float(CAM["mbf"])
        if forward:                                       # the plane x = 0 of KF1 holds both centres: kp2.y = small, the line is a column
            y1 = SCAN_FORWARD[1] + (small - float(CAM["cy"])) / float(CAM["fy"]) * (z - SCAN_FORWARD[2])
            X = to_world(T1, [0.0, y1, z])[0]
        elif kind == "epipolar":
            X = from_pixel(T2, 600.0 - 40 * variant, small, z)
        elif kind == "reproj1_stereo":
            X = from_pixel(T1, small + mbf / z, 150.0 + 10 * variant, z)
        else:
            X = from_pixel(T2, small + mbf / z, 150.0 + 10 * variant, z)
        u1, v1, z1 = project(T1, X); u2, v2, z2 = project(T2, X)
        u1, v1, z1, u2, v2, z2 = F32(u1[0]), F32(v1[0]), F32(z1[0]), F32(u2[0]), F32(v2[0]), F32(z2[0])
        ur1, ur2 = F32(u1 - CAM["mbf"] / z1), F32(u2 - CAM["mbf"] / z2)
        idn = D.identity(j % 8, j // 8)
        cd = D.candidate(idn, 5)
        if kind == "epipolar":
            A.add(u1, v1, idn); B.add(u2, val, cd)
        elif kind == "reproj1_mono":
            A.add(u1, v1, idn); B.add(u2, val, cd, stereo_z=z2)
        elif kind == "reproj1_stereo":
            A.add(u1, v1, idn, stereo_z=z1, ur=val); B.add(u2, v2, cd)
        elif kind == "reproj2_stereo":
            A.add(u1, v1, idn); B.add(u2, v2, cd, stereo_z=z2, ur=val)
        else:
            A.add(u1, v1, idn, stereo_z=z1); B.add(u2, val, cd)
        good.append({"epipolar": v2, "reproj1_mono": v2, "reproj1_stereo": ur1, "reproj2_stereo": ur2, "reproj2_mono": v2}[kind])
    return A.build(), B.build(), good


def scan_accepted(kind, kf1, kf2, contract="off"):
    """Per feature of kf1: matched (epipolar) / created (the others)."""
    if kind == "epipolar":
        return search(kf1, kf2, contract=contract)["match"] >= 0
    r = create(kf1, [kf2], contract=contract)
    ok = np.zeros(len(kf1["kp"]), bool); ok[r["new"]["idx1"]] = True
    return ok


def scan_case(voc, voc_oracle, kind, steps=512):
    """`steps` pairs in SCAN_WINDOWS windows: in each the sliding coordinate takes consecutive f32 values centred on the bound `kind`
    names, for a geometry of its own.  The windows are placed by bisection with the ORACLE (the reference), all windows at once; the
    device never takes part."""
    D = Descriptors(voc, 77)
    W = SCAN_WINDOWS

    def accepted(vals):
        kf1, kf2, _ = _scan_rows(kind, list(enumerate(vals)), D)
        attach_bow([kf1, kf2], voc_oracle)
        return scan_accepted(kind, kf1, kf2)

    good = np.array(_scan_rows(kind, [(v, F32(0)) for v in range(W)], D)[2], F32)
    assert np.all(good > 0), "the bisection walks the integer view of positive floats"
    lo, hi = good.copy(), (good + F32(8)).astype(F32)
    assert accepted(lo).all() and not accepted(hi).any(), kind
    while np.any(hi.view(np.int32) - lo.view(np.int32) > 1):
        mid = ((lo.view(np.int32).astype(np.int64) + hi.view(np.int32)) // 2).astype(np.int32).view(F32)
        ok = accepted(mid)
        lo, hi = np.where(ok, mid, lo).astype(F32), np.where(ok, hi, mid).astype(F32)
    per = steps // W
    items = [(v, x) for v in range(W) for x in (int(lo[v].view(np.int32)) - per // 2 + 1 + np.arange(per, dtype=np.int32)).astype(np.int32).view(F32)]
    kf1, kf2, _ = _scan_rows(kind, items, D)
    attach_bow([kf1, kf2], voc_oracle)
    return dict(name="scan_" + kind, kf1=kf1, neighbours=[kf2], median_depth=None, want=None, notes={})


def random_scene(voc, seed, n_points, n_neighbours, mono_share=0.4, noise=0.5, lv=None, cam=CAM, median=False, n_slots=8):
    """A synthetic two-view scene per neighbour: points 4 - 40 m in front of KF1 seen by both, mixed stereo / mono, `noise` px of
    Gaussian pixel noise (times the level's scale), descriptor distance 0 - 60, features in random order, some with map points."""
    rng = np.random.default_rng(7000 + 97 * seed + n_points + 13 * n_neighbours)
    lv = lv or Levels()
    D = Descriptors(voc, 500 + seed)
    T1 = pose(rodrigues(rng.normal(size=3) * 0.1), rng.normal(size=3))
    z = rng.uniform(4, 40, n_points); x = rng.uniform(-0.6, 0.6, n_points) * z; y = rng.uniform(-0.2, 0.2, n_points) * z
    Xw = to_world(T1, np.stack([x, y, z], 1))
    count = {}                                              # identity(slot, k) grows a pool per slot
    idents = []
    for i in range(n_points):
        s = int(rng.integers(0, n_slots)); count[s] = count.get(s, 0) + 1
        idents.append(D.identity(s, count[s] - 1))

    def view(T, share_seen):
        B = KeyFrameBuilder(T)
        order = rng.permutation(n_points)
        for i in order:
            if rng.random() > share_seen:
                continue
            u, v, zc = project(T, Xw[i])
            if zc[0] <= 0.5:
                continue
            octave = int(rng.integers(0, lv.nlevels))
            s = float(lv.scale[octave])
            u = u[0] + rng.normal() * noise * s; v = v[0] + rng.normal() * noise * s
            stereo = rng.random() > mono_share
            B.add(u, v, D.candidate(idents[i], int(rng.integers(0, 61))), octave, float(rng.uniform(0, 360)),
                  stereo_z=zc[0] * (1 + rng.normal() * 0.01) if stereo else None, has_mp=rng.random() < 0.1)
        return B.build()

    kf1 = view(T1, 1.0)
    nbs, med = [], []
    for k in range(n_neighbours):
        c = rng.normal(size=3) * (0.15 if k % 4 == 3 else 0.8)
        nbs.append(view(neighbour_pose(T1, c, rng.normal(size=3) * 0.03), 0.8))
        med.append(float(rng.choice([15.0, 200.0])))
    return dict(name="random_%d_%d_%d" % (seed, n_points, n_neighbours), kf1=kf1, neighbours=nbs, median_depth=med if median else None, want=None, notes={})


# ---------------------------------------------------------------- the device side (tests marked gpu, tools)
class Workspace:
    """n_slots image slots whose key points, descriptors, counts, uRight and depth the tests overwrite."""

    def __init__(self, fe, n_slots, voc, g=GEOM):
        import torch
        self.fe, self.n = fe, n_slots
        self.ex = fe.ORBextractor(g["nfeatures"], g["scale"], g["nlevels"], 20, 7)
        self.lv = Levels(g["scale"], g["nlevels"])
        assert self.lv.scale.tobytes() == self.ex.mvScaleFactor.tobytes() and self.lv.sigma2.tobytes() == self.ex.mvLevelSigma2.tobytes()
        self.b = fe.Batch(self.ex, g["W"], g["H"], n_slots)
        kp_p, desc_p, cnt_p, self.cap = self.b.results_device()
        ur_p, dep_p, _ = self.b.stereo_device()
        n = n_slots
        self.kp = fe.as_torch_u8(kp_p, n * self.cap * KP_DTYPE.itemsize).view(n, self.cap * KP_DTYPE.itemsize)
        self.desc = fe.as_torch_u8(desc_p, n * self.cap * 32).view(n, self.cap * 32)
        self.count = fe.as_torch_u8(cnt_p, n * 4).view(torch.int32)
        self.ur = fe.as_torch_u8(ur_p, n * self.cap * 4).view(torch.float32).view(n, self.cap)
        self.depth = fe.as_torch_u8(dep_p, n * self.cap * 4).view(torch.float32).view(n, self.cap)
        self.V = fe.Vocabulary.from_nodes(voc)
        self.b.extract_host(np.full((n, g["H"], g["W"]), 128, np.uint8))            # the images only make the slots valid
        self.b.sync()

    def close(self):
        self.V.close(); self.b.close()

    def upload(self, kfs, first=0, levelsup=LEVELSUP):
        """Keyframe j of `kfs` overwrites slot first + j; ComputeBoW runs on the written descriptors."""
        import torch
        assert first + len(kfs) <= self.n
        for j, f in enumerate(kfs):
            s, k = first + j, f["kp"]
            assert len(k) <= self.cap and (len(k) == 0 or int(k["octave"].max()) < self.lv.nlevels)
            if len(k):
                self.kp[s, :k.nbytes] = torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).cuda()
                self.desc[s, :f["desc"].size] = torch.from_numpy(f["desc"].reshape(-1).copy()).cuda()
                self.ur[s, :len(k)] = torch.from_numpy(f["ur"].copy()).cuda()
                self.depth[s, :len(k)] = torch.from_numpy(f["depth"].copy()).cuda()
            self.count[s] = len(k)
        torch.cuda.synchronize()
        self.b.compute_bow(self.V, list(range(first, first + len(kfs))), levelsup)
        self.b.sync()

    def has_table(self, kfs):
        """[len(kfs)][cap] u8 on the device (kept alive by the caller), or None when no keyframe has a map point."""
        import torch
        if all(k.get("has_mp") is None for k in kfs):
            return None
        t = np.zeros((len(kfs), self.cap), np.uint8)
        for j, k in enumerate(kfs):
            if k.get("has_mp") is not None:
                t[j, :len(k["has_mp"])] = k["has_mp"]
        return torch.from_numpy(t).cuda()
