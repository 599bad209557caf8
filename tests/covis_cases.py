"""Shared by test_covis_oracle.py, test_gpu_covis.py, tools/fuzz_covis.py and tools/bench_covis.py: the CPU oracle of the device covisibility
graph (tests/cpp/covis_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory), a restatement of the three
functions in the parallel terms of DESIGN.md Q43 (the observation relation derived from the keyframe tables, never stored), the runner that
plays a script through sd_covis_*, and the crafted cases.

A script is a list of operations on one graph:
    ("add", kf, octave u8[n], uright f32[n], depth f32[n], protected)
    ("match", [kf], [idx], [mp])   ("bad", [mp], [0/1])   ("parent", [kf], [parent])   ("erase", [kf])   ("update", [kf])
    ("conn", kf, best_n, min_weight)   ("cull", [cand], [not_erase] or None, monocular, th_depth)   ("local", [frame: point ids])
Every runner returns one item per conn / cull / local operation, followed by the connections of every keyframe the script named.  All
items are plain Python / bytes so that == is the byte-for-byte comparison."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32, U8 = np.float32, np.int32, np.uint8
BRANCHES = ["uc_empty", "uc_self", "uc_bad_point", "uc_null_point", "uc_w14", "uc_w15", "uc_w16", "uc_none_kept", "uc_tied_max", "ac_absent", "ac_changed",
            "ac_equal", "ac_resort_mixed", "uc_first", "uc_protected", "er_connection", "cu_protected", "cu_bad", "cu_null", "cu_depth_far", "cu_depth_neg",
            "cu_depth_nan", "cu_depth_eq", "cu_obs3", "cu_obs4", "cu_oct_p1", "cu_oct_p2", "cu_others2", "cu_others3", "cu_on_bound", "cu_flagged",
            "cu_not_erase", "cu_removed_observer", "cu_point_driven_bad", "lm_empty", "lm_bad_entry", "lm_vote_tie", "lm_stop", "lm_at_80", "lm_neighbour",
            "lm_neighbour_dead", "lm_child", "lm_parent_break", "lm_dup_point", "lm_bad_local_point"]
TWINS = dict(none=0, th_gt=1, tie_asc=2, ac_no_early=3, ac_kept_only=4, cull_unweighted=5, cull_static=6, lm_inner_break=7)

_oracle = None


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _buf(a, dt):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return a if len(a) else np.zeros(1, dt)


def oracle():
    global _oracle
    if _oracle is None:
        d = tempfile.mkdtemp(prefix="covis_oracle_")
        so = os.path.join(d, "libcovis_oracle.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "cpp", "covis_oracle.cpp")])
        L = C.CDLL(so)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.sd_covis_oracle_branches.restype = C.POINTER(C.c_int64)
        L.sd_covis_oracle_set_twin.argtypes = [i]
        L.sd_covis_oracle_new.restype = vp
        L.sd_covis_oracle_free.argtypes = [vp]
        L.sd_covis_oracle_add.argtypes = [vp, i, i, vp, vp, vp, i]
        L.sd_covis_oracle_set_match.argtypes = [vp, i, i, i]
        L.sd_covis_oracle_set_bad.argtypes = [vp, i, i]
        L.sd_covis_oracle_set_parent.argtypes = [vp, i, i]
        L.sd_covis_oracle_erase.argtypes = [vp, i]
        L.sd_covis_oracle_update.argtypes = [vp, i]
        L.sd_covis_oracle_connections.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp]
        L.sd_covis_oracle_culling.argtypes = [vp, i, vp, vp, i, f, vp, i]
        L.sd_covis_oracle_clone.restype = vp
        L.sd_covis_oracle_clone.argtypes = [vp]
        L.sd_covis_oracle_local_map.argtypes = [vp, i, vp, vp, vp, vp, vp]
        assert L.sd_covis_oracle_branch_count() == len(BRANCHES)
        _oracle = L
    return _oracle


def branches():
    b = oracle().sd_covis_oracle_branches()
    return {name: int(b[i]) for i, name in enumerate(BRANCHES)}


# ---------------------------------------------------------------- records (plain, so that == compares everything)
def conn_record(live, n_features, prot, parent, first, ordered_id, ordered_weight, row_id, row_weight, n_best, n_by_weight):
    return ("conn", bool(live), int(n_features), bool(prot), int(parent), bool(first), [int(x) for x in ordered_id], [int(x) for x in ordered_weight],
            [int(x) for x in row_id], [int(x) for x in row_weight], int(n_best), int(n_by_weight))


def cull_record(rows):
    return ("cull", [(int(a), int(b), int(c)) for a, b, c in rows])


def local_record(local_kf, ref, pts, n_voted, entry_bad):
    return ("local", [int(x) for x in local_kf], int(ref), [int(x) for x in pts], int(n_voted), [int(x) for x in entry_bad])


def ids_of(ops):
    ids = set()
    for op in ops:
        if op[0] == "add":
            ids.add(int(op[1]))
    return sorted(ids)


def max_ids(ops):
    """(max_keyframes, max_features, max_points) a script needs."""
    kf = feat = pt = 0
    for op in ops:
        if op[0] == "add":
            kf = max(kf, op[1] + 1); feat += len(op[2])
        elif op[0] == "match" and len(op[3]):
            pt = max(pt, int(np.max(op[3])) + 1)
        elif op[0] == "bad" and len(op[1]):
            pt = max(pt, int(np.max(op[1])) + 1)
        elif op[0] == "local":
            for fr in op[1]:
                if len(fr):
                    pt = max(pt, int(np.max(fr)) + 1)
    return max(kf, 1), max(feat, 1), max(pt, 1)


# ---------------------------------------------------------------- the sequential oracle
class OracleGraph:
    def __init__(self, cap):
        self.L, self.cap = oracle(), cap
        self.h = self.L.sd_covis_oracle_new()

    def close(self):
        if self.h:
            self.L.sd_covis_oracle_free(self.h)
        self.h = None

    def connections(self, kf, best_n=10, min_weight=0):
        oi = np.zeros(self.cap, I32); ow = np.zeros(self.cap, I32); ri = np.zeros(self.cap, I32); rw = np.zeros(self.cap, I32); info = np.zeros(9, I32)
        self.L.sd_covis_oracle_connections(self.h, kf, best_n, min_weight, _p(oi), _p(ow), _p(ri), _p(rw), _p(info))
        return conn_record(info[0], info[1], info[2], info[3], info[4], oi[:info[5]], ow[:info[5]], ri[:info[6]], rw[:info[6]], info[7], info[8])

    def clone(self):
        g = OracleGraph.__new__(OracleGraph)
        g.L, g.cap, g.h = self.L, self.cap, self.L.sd_covis_oracle_clone(self.h)
        return g

    def culling(self, cand, not_erase, mono, th, in_place=False):
        c = _buf(cand, I32); ne = _buf(not_erase if not_erase is not None else np.zeros(len(cand)), U8); out = np.zeros(3 * max(len(cand), 1), I32)
        self.L.sd_covis_oracle_culling(self.h, len(cand), _p(c), _p(ne), int(bool(mono)), C.c_float(float(F32(th))), _p(out), int(in_place))
        return cull_record(out.reshape(-1, 3)[:len(cand)])

    def local_map(self, frame, max_points):
        fr = np.ascontiguousarray(frame, I32).reshape(-1); eb = np.zeros(max(len(fr), 1), U8)
        lk = np.zeros(self.cap + 4, I32); lp = np.zeros(max_points + 1, I32); info = np.zeros(6, I32)
        self.L.sd_covis_oracle_local_map(self.h, len(fr), _p(_buf(fr, I32)), _p(eb), _p(lk), _p(lp), _p(info))
        return local_record(lk[:info[0]], info[2], lp[:info[3]], info[1], eb[:len(fr)])


def run_oracle(ops, twin="none"):
    """The script through the sequential oracle -> (results, branches)."""
    L = oracle()
    L.sd_covis_oracle_reset_branches(); L.sd_covis_oracle_set_twin(TWINS[twin])
    K, _, P = max_ids(ops)
    g = OracleGraph(K)
    out = []
    try:
        for op in ops:
            if op[0] == "add":
                assert L.sd_covis_oracle_add(g.h, op[1], len(op[2]), _p(_buf(op[2], U8)), _p(_buf(op[3], F32)), _p(_buf(op[4], F32)), int(op[5])) == 0
            elif op[0] == "match":
                for k, i, m in zip(op[1], op[2], op[3]):
                    L.sd_covis_oracle_set_match(g.h, int(k), int(i), int(m))
            elif op[0] == "bad":
                for m, b in zip(op[1], op[2]):
                    L.sd_covis_oracle_set_bad(g.h, int(m), int(b))
            elif op[0] == "parent":
                for k, q in zip(op[1], op[2]):
                    L.sd_covis_oracle_set_parent(g.h, int(k), int(q))
            elif op[0] == "erase":
                for k in op[1]:
                    L.sd_covis_oracle_erase(g.h, int(k))
            elif op[0] == "update":
                for k in op[1]:
                    L.sd_covis_oracle_update(g.h, int(k))
            elif op[0] == "conn":
                out.append(g.connections(op[1], op[2], op[3]))
            elif op[0] == "cull":
                out.append(g.culling(op[1], op[2], op[3], op[4]))
            elif op[0] == "local":
                out.append([g.local_map(fr, P) for fr in op[1]])
        out.append([g.connections(k) for k in ids_of(ops)])
    finally:
        L.sd_covis_oracle_set_twin(0)
        g.close()
    return out, branches()


# ---------------------------------------------------------------- the restatement (in its parallel terms)
class NumpyGraph:
    """Tables only: per keyframe mp / octave / stereo / depth, per point a bad flag, the rows and lists.  Observers are found by scanning the
    tables, as the device's index by map point is."""

    def __init__(self):
        self.kf, self.bad = {}, {}

    def observers(self):
        obs = {}
        for k in sorted(self.kf):
            E = self.kf[k]
            if E["live"]:
                for i in np.nonzero(E["mp"] >= 0)[0]:
                    obs.setdefault(int(E["mp"][i]), []).append((k, int(i)))
        return obs

    @staticmethod
    def order(pairs):
        """[(id, w)] by descending (w, id)."""
        return sorted(pairs, key=lambda t: (t[1], t[0]), reverse=True)

    def resort(self, k):
        E = self.kf[k]
        o = self.order(list(E["row"].items()))
        E["ord"] = [(a, b) for a, b in o]

    def update(self, k):
        E = self.kf[k]
        obs = self.observers()
        cnt = {}
        for p in E["mp"][E["mp"] >= 0]:
            if not self.bad.get(int(p), False):
                for k2, _ in obs[int(p)]:
                    if k2 != k:
                        cnt[k2] = cnt.get(k2, 0) + 1
        if not cnt:
            return
        nmax = max(cnt.values())
        kmax = min(a for a, w in cnt.items() if w == nmax)
        kept = [(a, w) for a, w in cnt.items() if w >= 15] or [(kmax, nmax)]
        for a, w in sorted(kept):
            X = self.kf[a]
            if X["row"].get(k) != w:
                X["row"][k] = w
                self.resort(a)
        E["row"] = dict(cnt)
        E["ord"] = self.order(kept)
        if E["first"] and not E["prot"]:
            E["parent"] = E["ord"][0][0]; E["first"] = False

    def erase(self, k):
        E = self.kf.get(k)
        if E is None or not E["live"] or E["prot"]:
            return
        for a in list(E["row"]):
            if k in self.kf[a]["row"]:
                del self.kf[a]["row"][k]
                self.resort(a)
        E["mp"][:] = -1; E["row"] = {}; E["ord"] = []; E["live"] = False

    def connections(self, k, best_n=10, min_weight=0):
        E = self.kf[k]
        ow = [w for _, w in E["ord"]]
        nw = sum(1 for w in ow if w >= min_weight)
        row = sorted(E["row"].items())
        return conn_record(E["live"], len(E["mp"]), E["prot"], E["parent"] if E["live"] else -1, E["first"], [a for a, _ in E["ord"]], ow, [a for a, _ in row],
                           [w for _, w in row], min(len(ow), max(best_n, 0)), 0 if nw == len(ow) else nw)

    def culling(self, cand, not_erase, mono, th):
        obs = self.observers()
        th = F32(th)
        removed, rows = set(), []
        for c, k in enumerate(cand):
            E = self.kf[k]
            if E["prot"]:
                rows.append((0, 0, 0)); continue
            nmps = nred = 0
            for i in np.nonzero(E["mp"] >= 0)[0]:
                p = int(E["mp"][i])
                if self.bad.get(p, False):
                    continue
                d = E["depth"][i]
                if not mono and (d > th or d < F32(0)):
                    continue
                left = [(k2, i2) for k2, i2 in obs[p] if k2 not in removed]
                w = sum(2 if self.kf[k2]["stereo"][i2] else 1 for k2, i2 in left)
                if len(left) < len(obs[p]) and w <= 2:
                    continue
                nmps += 1
                fine = sum(1 for k2, i2 in left if k2 != k and int(self.kf[k2]["oct"][i2]) <= int(E["oct"][i]) + 1)
                if w > 3 and fine >= 3:
                    nred += 1
            flag = float(nred) > 0.9 * float(nmps)
            rows.append((int(flag), nmps, nred))
            if flag and not (not_erase is not None and not_erase[c]):
                removed.add(k)
        return cull_record(rows)

    def local_map(self, frame):
        obs = self.observers()
        votes, eb = {}, []
        for p in frame:
            p = int(p)
            b = p >= 0 and self.bad.get(p, False)
            eb.append(int(b))
            if p >= 0 and not b:
                for k2, _ in obs.get(p, []):
                    votes[k2] = votes.get(k2, 0) + 1
        if not votes:
            return local_record([], -1, [], 0, eb)
        local = sorted(votes)
        top = max(votes.values())
        ref = min(k for k in local if votes[k] == top)
        inc = set(local)
        n_first = len(local)
        for m in range(n_first):
            if len(local) > 80:
                break
            k = local[m]
            E = self.kf[k]
            for a, _ in E["ord"][:10]:
                if self.kf[a]["live"] and a not in inc:
                    local.append(a); inc.add(a); break
            ch = [a for a in sorted(self.kf) if a != k and self.kf[a]["live"] and self.kf[a]["parent"] == k and a not in inc]
            if ch:
                local.append(ch[0]); inc.add(ch[0])
            if E["parent"] >= 0 and E["parent"] not in inc:
                local.append(E["parent"]); inc.add(E["parent"])
                break
        first = {}
        for pos, k in enumerate(local):
            E = self.kf.get(k)
            if E is not None and E["live"]:
                for i in np.nonzero(E["mp"] >= 0)[0]:
                    p = int(E["mp"][i])
                    if not self.bad.get(p, False) and p not in first:
                        first[p] = (pos, int(i))
        pts = sorted(first, key=lambda p: first[p])
        return local_record(local, ref, pts, n_first, eb)


def run_numpy(ops):
    g = NumpyGraph()
    out = []
    for op in ops:
        if op[0] == "add":
            assert op[1] not in g.kf or not g.kf[op[1]]["live"]
            n = len(op[2])
            g.kf[op[1]] = dict(live=True, prot=bool(op[5]), mp=np.full(n, -1, I32), oct=np.asarray(op[2], U8).copy(), stereo=np.asarray(op[3], F32) >= 0,
                               depth=np.asarray(op[4], F32).copy(), parent=-1, first=True, row={}, ord=[])
        elif op[0] == "match":
            for k, i, m in zip(op[1], op[2], op[3]):
                g.kf[int(k)]["mp"][int(i)] = int(m)
        elif op[0] == "bad":
            for m, b in zip(op[1], op[2]):
                g.bad[int(m)] = bool(b)
        elif op[0] == "parent":
            for k, q in zip(op[1], op[2]):
                g.kf[int(k)]["parent"] = int(q)
        elif op[0] == "erase":
            for k in op[1]:
                g.erase(int(k))
        elif op[0] == "update":
            for k in op[1]:
                g.update(int(k))
        elif op[0] == "conn":
            out.append(g.connections(op[1], op[2], op[3]))
        elif op[0] == "cull":
            out.append(g.culling(op[1], op[2], op[3], op[4]))
        elif op[0] == "local":
            out.append([g.local_map(fr) for fr in op[1]])
    out.append([g.connections(k) for k in ids_of(ops)])
    return out


# ---------------------------------------------------------------- the device
def device_conn(g, kf, best_n=10, min_weight=0):
    c = g.connections(kf, best_n, min_weight)
    return conn_record(c["live"], c["n_features"], c["is_protected"], c["parent"], c["first_connection"], c["ordered_id"], c["ordered_weight"], c["row_id"],
                       c["row_weight"], len(c["best"]), len(c["by_weight"]))


def run_device(fe, ops, max_kf=None, max_jobs=None, max_local_points=None, device=False, graph=None, device_matches=False):
    """The script through sd_covis_* (frontend.CovisibilityGraph).  device=True sends local-map frames through the device-array entry point, device_matches=True the matches."""
    K, F, P = max_ids(ops)
    K = max(K, max_kf or 0)
    jobs = max([len(op[1]) for op in ops if op[0] in ("update", "cull", "local")] + [1])
    g = graph or fe.CovisibilityGraph(K, F, P, max(jobs, max_jobs or 0), max_local_points or max(F, 1))
    out = []
    try:
        for op in ops:
            if op[0] == "add":
                g.add_host(op[1], op[2], op[3], op[4], op[5])
            elif op[0] == "match" and device_matches:
                last = {}
                for k, f, m in zip(op[1], op[2], op[3]):
                    last[(int(k), int(f))] = int(m)               # the device path takes every feature once
                g.set_matches_device([k for k, _ in last], [f for _, f in last], list(last.values()))
            elif op[0] == "match":
                g.set_matches(op[1], op[2], op[3])
            elif op[0] == "bad":
                g.set_point_bad(op[1], np.asarray(op[2], U8))
            elif op[0] == "parent":
                g.set_parent(op[1], op[2])
            elif op[0] == "erase":
                g.erase(op[1])
            elif op[0] == "update":
                g.update_connections(op[1])
            elif op[0] == "conn":
                out.append(device_conn(g, op[1], op[2], op[3]))
            elif op[0] == "cull":
                r = g.keyframe_culling(op[1], op[2], op[3], op[4])
                out.append(cull_record([(x["flag"], x["n_mps"], x["n_redundant"]) for x in r]))
            elif op[0] == "local":
                r = g.local_map(op[1], device=device)
                out.append([local_record(x["local_kf"], x["reference_kf"], x["local_points"], x["info"]["n_voted"], x["entry_bad"]) for x in r])
        out.append([device_conn(g, k) for k in ids_of(ops)])
    finally:
        if graph is None:
            g.close()
    return out


def assert_same(got, want, what):
    assert len(got) == len(want), "%s: %d results, %d expected" % (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
                for j, (x, y) in enumerate(zip(a, b)):
                    assert x == y, "%s: result %d item %d differs:\n got  %r\n want %r" % (what, i, j, x, y)
            raise AssertionError("%s: result %d differs:\n got  %r\n want %r" % (what, i, a, b))


def differs(a, b):
    return a != b


# ---------------------------------------------------------------- building scripts
class Builder:
    """Keyframes with plain features (octave 0, monocular, depth 1) unless said otherwise; a new point takes the next free feature of every
    keyframe that observes it."""

    def __init__(self):
        self.ops, self.free, self.n, self.next_point = [], {}, {}, 0

    def kf(self, k, n=64, octave=0, uright=-1.0, depth=1.0, prot=False):
        o = np.broadcast_to(np.asarray(octave, U8), (n,)).copy(); u = np.broadcast_to(np.asarray(uright, F32), (n,)).copy()
        d = np.broadcast_to(np.asarray(depth, F32), (n,)).copy()
        self.ops.append(("add", k, o, u, d, prot))
        self.free[k] = 0; self.n[k] = n
        return self

    def point(self, observers, at=None):
        """A new point seen by `observers`; at = {kf: feature index} overrides the next free feature."""
        p = self.next_point
        self.next_point += 1
        self.see(p, observers, at)
        return p

    def see(self, p, observers, at=None):
        kk, ii = [], []
        for k in observers:
            i = (at or {}).get(k)
            if i is None:
                i = self.free[k]; self.free[k] += 1
            assert i < self.n[k], "keyframe %d is full" % k
            kk.append(k); ii.append(i)
        self.ops.append(("match", kk, ii, [p] * len(kk)))

    def share(self, a, b, n):
        return [self.point([a, b]) for _ in range(n)]

    def op(self, *o):
        self.ops.append(tuple(o))
        return self


def case(name, ops, claims, twin=None):
    return dict(name=name, ops=ops, claims=claims, twin=twin)


def crafted_cases():
    cs = []
    # ---- UpdateConnections
    b = Builder()
    b.kf(0, prot=True)
    for k in (1, 2, 3, 4):
        b.kf(k)
    for k, w in ((1, 14), (2, 15), (3, 16)):
        b.share(k, 4, w)
    b.op("update", [4]).op("conn", 4, 1, 15).op("conn", 4, 10, 16).op("conn", 4, 0, 17)
    cs.append(case("weights_14_15_16", b.ops, ["uc_w14", "uc_w15", "uc_w16", "uc_self", "uc_null_point", "ac_absent", "uc_first"], "th_gt"))

    b = Builder()
    for k in (1, 2, 3, 5):
        b.kf(k)
    b.share(2, 5, 5); b.share(1, 5, 5); b.share(3, 5, 4)
    b.op("update", [5])
    cs.append(case("none_kept_tied_maxima", b.ops, ["uc_none_kept", "uc_tied_max"]))

    b = Builder()
    b.kf(1).kf(2).kf(3, n=0)
    pts = b.share(1, 2, 3)
    b.op("bad", pts, [1, 1, 1]).op("update", [1, 3]).op("conn", 1, 10, 0)
    b.op("bad", pts[:1], [0]).op("update", [1])
    cs.append(case("empty_counter_and_bad_points", b.ops, ["uc_empty", "uc_bad_point", "uc_none_kept"]))

    b = Builder()
    for k in (1, 2, 3, 7):
        b.kf(k, n=80)
    for k in (2, 1, 3):
        b.share(k, 7, 20)
    b.op("update", [7]).op("conn", 7, 2, 20).op("conn", 7, 2, 21)
    cs.append(case("tie_order_descending_id", b.ops, ["uc_w16"], "tie_asc"))

    b = Builder()
    b.kf(1, n=80).kf(4, n=80)
    b.share(1, 4, 16)
    b.op("update", [4]).op("update", [4]).op("conn", 1, 10, 0)
    b.share(1, 4, 2)
    b.op("update", [4]).op("update", [1])
    cs.append(case("add_connection_equal_changed_absent", b.ops, ["ac_absent", "ac_equal", "ac_changed"]))

    b = Builder()
    for k in (1, 2, 3, 4):
        b.kf(k, n=80)
    b.share(1, 2, 20); b.share(1, 3, 3); b.share(1, 4, 16)
    b.op("update", [1]).op("conn", 1, 10, 0)
    b.op("update", [2]).op("conn", 1, 10, 0)                # AddConnection(1 <- 2, 20): equal, the list of 1 stays the kept pairs
    b.op("update", [4]).op("conn", 1, 10, 0)                # 1 already holds 4 with 16: equal again
    b.share(1, 4, 1)
    b.op("update", [4]).op("conn", 1, 10, 0).op("conn", 1, 10, 15).op("conn", 1, 10, 3)     # changed: the list of 1 is rebuilt from its whole row, 3 included
    cs.append(case("resort_mixes_entries_below_15", b.ops, ["ac_resort_mixed", "ac_equal", "ac_changed"], "ac_kept_only"))

    b = Builder()
    for k in (1, 2, 3):
        b.kf(k, n=80)
    b.share(1, 2, 20); b.share(1, 3, 3)
    b.op("update", [1]).op("update", [2]).op("conn", 1, 10, 0)
    cs.append(case("early_return_keeps_the_kept_list", b.ops, ["ac_equal"], "ac_no_early"))

    b = Builder()
    b.kf(0, prot=True).kf(1).kf(2)
    b.share(0, 1, 20); b.share(0, 2, 16)
    b.op("update", [0]).op("update", [1])
    b.share(1, 2, 30)
    b.op("update", [1]).op("update", [2, 0]).op("erase", [0])
    cs.append(case("first_connection_and_protected", b.ops, ["uc_first", "uc_protected"]))

    b = Builder()
    for k in (1, 2, 3, 4):
        b.kf(k, n=100)
    b.share(1, 2, 20); b.share(1, 3, 18); b.share(2, 3, 16); b.share(3, 4, 5); b.share(1, 4, 15)
    b.op("update", [1, 2, 3, 4]).op("erase", [1]).op("conn", 2, 10, 0).op("update", [2, 3]).op("parent", [2, 3, 4], [3, -1, 3])
    b.kf(1, n=10)
    b.share(1, 4, 6)
    b.op("update", [1, 4])
    cs.append(case("erase_then_update_then_readd", b.ops, ["er_connection", "uc_first"]))

    b = Builder()
    for k in (1, 2, 3):
        b.kf(k, n=100)
    b.share(1, 2, 20); b.share(2, 3, 17); b.share(1, 3, 15)
    b.op("update", [3, 1, 2]).op("update", [2, 2, 1])
    cs.append(case("several_in_one_call_in_list_order", b.ops, ["ac_equal"]))

    # ---- KeyFrameCulling
    def others(b, c, n_points, n_others, pool, stereo_pool=None):
        """n_points new points seen by c and by the first n_others keyframes of pool."""
        return [b.point([c] + list(pool[:n_others])) for _ in range(n_points)]

    b = Builder()
    b.kf(0, prot=True, n=40)
    for k in range(1, 7):
        b.kf(k, n=40)
    b.kf(7, n=40, uright=5.0).kf(8, n=40, uright=5.0).kf(9, n=40, uright=5.0)
    others(b, 1, 4, 2, [2, 3, 4])            # Observations() = 3, mono
    others(b, 1, 4, 3, [2, 3, 4])            # 4, mono, three others: redundant
    b.point([1, 7])                          # 1 + 2 = 3 with a stereo observer
    b.point([1, 7, 5])                       # 4 with a stereo observer, two others
    b.point([9, 7]); b.point([9, 7, 8, 2])   # a stereo candidate: 4 with one other, 7 with three
    others(b, 0, 5, 3, [2, 3, 4])
    b.op("cull", [1, 9, 0, 2], None, True, 0.0)
    cs.append(case("observations_3_4_mono_stereo", b.ops, ["cu_obs3", "cu_obs4", "cu_others2", "cu_others3", "cu_protected", "cu_null"]))

    b = Builder()
    b.kf(1, n=8, octave=2)
    b.kf(2, n=8, octave=3).kf(3, n=8, octave=3).kf(4, n=8, octave=[3, 4, 4, 4, 4, 4, 4, 4]).kf(5, n=8, octave=0)
    b.point([1, 2, 3, 4])                    # level + 1 three times: redundant
    b.point([1, 2, 3, 4])                    # the third at level + 2: two fine observers
    b.point([1, 5, 2, 4])                    # coarser is fine too: octave 0, 3 and ... 4 is not
    b.op("cull", [1], None, True, 0.0)
    cs.append(case("octave_plus_1_plus_2", b.ops, ["cu_oct_p1", "cu_oct_p2", "cu_others2", "cu_others3"]))

    th = F32(40.0)
    up, down = np.nextafter(th, F32(np.inf)), np.nextafter(th, F32(0))
    b = Builder()
    b.kf(1, n=8, depth=[th, up, down, -1.0, np.nan, -0.0, np.inf, 1.0], uright=3.0)
    for k in (2, 3, 4):
        b.kf(k, n=8)
    for _ in range(8):
        b.point([1, 2, 3, 4])
    pts = list(range(8))
    b.op("cull", [1], None, False, th).op("cull", [1], None, True, th).op("bad", pts[:1], [1]).op("cull", [1], None, False, th)
    cs.append(case("depth_on_the_threshold", b.ops, ["cu_depth_eq", "cu_depth_far", "cu_depth_neg", "cu_depth_nan", "cu_bad"]))

    for n in (10, 20, 30):
        b = Builder()
        for k in (1, 2, 3):
            b.kf(k, n=3 * n + 3)
        cand = []
        for j, d in enumerate((-1, 0, 1)):
            c = 10 + j
            cand.append(c)
            b.kf(c, n=n)
            others(b, c, 9 * n // 10 + d, 3, [1, 2, 3])
            others(b, c, n - 9 * n // 10 - d, 1, [1, 2, 3])
        b.op("cull", cand, [1, 1, 1], True, 0.0)
        cs.append(case("bound_0.9_of_%d" % n, b.ops, ["cu_on_bound", "cu_flagged", "cu_not_erase"]))

    for ne in (None, [1, 0]):
        b = Builder()
        for k in (1, 2, 3, 4):
            b.kf(k, n=20)
        for _ in range(10):
            b.point([1, 2, 3, 4])            # for 1: others 2, 3, 4.  Once 1 is gone, 2 sees Observations() = 3
        b.op("cull", [1, 2], ne, True, 0.0).op("cull", [2, 1], ne, True, 0.0)
        cs.append(case("first_removal_saves_the_second" + ("_not_erase" if ne else ""), b.ops, ["cu_flagged"] + (["cu_not_erase"] if ne else ["cu_removed_observer"]),
                       None if ne else "cull_static"))

    b = Builder()
    for k in (1, 2, 3, 4, 5, 6):
        b.kf(k, n=30)
    others(b, 1, 10, 3, [3, 4, 5])           # 1 is redundant ...
    for _ in range(1):
        b.point([1, 2, 6])                   # ... and this point, with three mono observers, goes bad when 1 is removed
    others(b, 2, 9, 3, [3, 4, 5])            # 2: nine redundant of ten if that point still counted (not flagged), of nine without it (flagged)
    b.op("cull", [1, 2], None, True, 0.0).op("cull", [1, 2], [1, 0], True, 0.0)
    cs.append(case("point_driven_bad_by_a_removal", b.ops, ["cu_point_driven_bad", "cu_removed_observer"], "cull_static"))

    b = Builder()
    for k in (1, 2, 3, 4, 5):
        b.kf(k, n=30, uright=2.0)
    others(b, 1, 10, 3, [3, 4, 5])
    b.point([1, 2, 3])                       # three stereo observers: 6, and 4 without keyframe 1 -- still good; an unweighted count of 2 would be bad
    others(b, 2, 9, 3, [3, 4, 5])
    b.op("cull", [1, 2], None, True, 0.0)
    cs.append(case("weighted_observations_after_a_removal", b.ops, ["cu_removed_observer"], "cull_unweighted"))

    # ---- UpdateLocalKeyFrames / UpdateLocalPoints
    b = Builder()
    for k in (1, 2, 3):
        b.kf(k, n=20)
    a = b.share(1, 3, 3); c = b.share(2, 3, 3); d = b.point([2])
    b.op("bad", [d], [1])
    b.op("local", [a + c + [d, -1], [d, -1, -1], [], a[:1]])
    cs.append(case("votes_tie_and_bad_entries", b.ops, ["lm_vote_tie", "lm_bad_entry", "lm_empty", "lm_dup_point", "lm_bad_local_point"]))

    b = Builder()
    for k in range(1, 8):
        b.kf(k, n=60)
    b.share(1, 2, 20); b.share(1, 3, 16); b.share(4, 5, 15); b.share(6, 7, 15); b.share(4, 3, 15)
    b.op("update", [1, 2, 3, 4, 5, 6, 7]).op("parent", [1, 4, 5, 3, 6], [6, 1, 1, -1, -1])
    own1 = b.point([1]); own4 = b.point([4]); own5 = b.point([5])
    b.op("local", [[own1], [own4], [own5, own4], [own1, own4]])
    cs.append(case("neighbour_child_parent_and_the_break", b.ops, ["lm_neighbour", "lm_child", "lm_parent_break"], "lm_inner_break"))

    for n_first in (79, 80, 81):
        b = Builder()
        frame = []
        for k in range(n_first):
            b.kf(k, n=20)
            frame.append(b.point([k]))
        for k in range(n_first):
            b.kf(100 + k, n=20)
            b.share(k, 100 + k, 15)
        b.op("update", list(range(n_first))).op("local", [frame])
        cs.append(case("stop_test_with_%d_voted" % n_first, b.ops, ["lm_stop"] + (["lm_at_80"] if n_first == 80 else []) + (["lm_neighbour"] if n_first < 81 else [])))

    b = Builder()
    b.kf(1, n=40).kf(2, n=40).kf(3, n=40)
    sh = b.share(1, 2, 16); b.share(1, 3, 15)
    b.op("update", [1])
    b.op("match", [2] * 16, list(range(16)), [-1] * 16)       # 2 no longer shares anything with 1 ...
    b.point([2, 3])
    b.op("update", [2]).op("erase", [2])                     # ... so its row does not name 1, and its erase leaves 1's list pointing at it
    own1 = b.point([1])
    b.op("conn", 1, 10, 0).op("local", [[own1]])
    cs.append(case("a_dead_neighbour_is_skipped", b.ops, ["lm_neighbour_dead", "lm_neighbour", "uc_none_kept"]))
    return cs


# ---------------------------------------------------------------- shapes and random maps
def shape_script(n_kf, n_feat, observers_of_point=None):
    """n_kf keyframes of n_feat features; point j is seen at feature j by keyframes j % n_kf .. (a window of 3), so that every kernel walks
    every keyframe; update, cull and local map over the first few."""
    b = Builder()
    for k in range(n_kf):
        b.kf(k, n=n_feat, uright=(1.0 if k % 3 == 0 else -1.0), octave=k % 4)
    frame = []
    for j in range(n_feat):
        obs = sorted({(j + d) % n_kf for d in range(3)}) if observers_of_point is None else list(range(min(observers_of_point, n_kf)))
        if obs:
            frame.append(b.point(obs, at={k: j for k in obs}))
    some = list(range(min(n_kf, 5)))
    b.op("update", some).op("cull", some, None, False, 35.0).op("local", [frame[::2], frame[:1]])
    return b.ops


def random_script(seed, n_kf=40, n_feat=60, n_points=400, rounds=4):
    rng = np.random.default_rng(seed)
    b = Builder()
    live = []
    table = {}

    def add(k):
        b.kf(k, n=n_feat, octave=rng.choice([0, 1, 2, 6], n_feat, p=[0.8, 0.16, 0.02, 0.02]), uright=np.where(rng.random(n_feat) < 0.4, 3.0, -1.0), depth=rng.choice([1.0, 50.0, -1.0], n_feat, p=[0.8, 0.15, 0.05]),
             prot=(k == 0))
        live.append(k); table[k] = np.full(n_feat, -1)

    for k in range(n_kf):
        add(k)
    for r in range(rounds):
        kk, ii, mm = [], [], []
        for p in rng.permutation(n_points)[:n_points * 3 // 4]:
            centre = int(rng.integers(0, len(live)))
            for k in {live[(centre + int(d)) % len(live)] for d in rng.integers(0, 8, int(rng.integers(6, 14)))}:
                if p in table[k]:
                    continue
                i = int(rng.integers(0, n_feat))
                table[k][i] = p
                kk.append(k); ii.append(i); mm.append(int(p))
        b.op("match", kk, ii, mm)
        bad = rng.permutation(n_points)[:10]
        b.op("bad", [int(x) for x in bad], [int(x) for x in rng.integers(0, 2, 10)])
        order = [int(x) for x in rng.permutation(live)]
        b.op("update", order[:len(order) // 2]).op("update", order[len(order) // 2:])
        cand = [int(x) for x in rng.permutation(live)[:12]]
        b.op("cull", cand, [int(x) for x in rng.integers(0, 2, len(cand))], bool(r & 1), 40.0)
        frames = [np.where(rng.random(80) < 0.2, -1, rng.integers(0, n_points, 80)) for _ in range(3)]
        b.op("local", frames)
        gone = [int(x) for x in rng.permutation([k for k in live if k != 0])[:min(3, max(len(live) - 6, 0))]]
        b.op("erase", gone)
        for k in gone:
            live.remove(k); table[k][:] = -1
        b.op("parent", [int(k) for k in live if k != 0][:5], [int(rng.choice(live)) for _ in range(min(5, len(live) - 1))])
        b.op("conn", live[1], 5, int(rng.integers(1, 30)))
    b.op("update", live)
    return b.ops
