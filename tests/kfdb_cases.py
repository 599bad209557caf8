"""Shared by test_kfdb_oracle.py, test_gpu_kfdb.py, tools/fuzz_kfdb.py and tools/bench_kfdb.py: the CPU oracle of the device KeyFrameDatabase
(tests/cpp/kfdb_oracle.cpp, compiled with g++ -O2 -ffp-contract=off into a temporary directory), a numpy restatement of the two queries in
the parallel terms of DESIGN.md Q42, the runner that plays a script through sd_kfdb_*, and the crafted cases.

A script is a list of operations on one database:
    ("add", kf_id, word, value)   ("erase", kf_id)   ("cov", kf_id, [neighbour ids])   ("clear",)
    ("loop", [queries], [min_score], [excluded ids per query] or None)   ("reloc", [queries])   ("score", [queries], [listed ids per query])
with a query = (word u32 ascending, value f64).  Every runner returns one item per loop / reloc / score operation: a list with one record
per query -- dict(candidates i32, info INFO_DTYPE, sharing MEMBER_DTYPE, acc ACC_DTYPE), or for score an f32 array -- followed by the
entries' final (seq, live, reloc_score).  With one shared word and positive values a score is exactly min(v, w), with several the sum of the
minima: every threshold below is hit with powers of two."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32
INFO_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common_words", "<i4"), ("min_common_words", "<i4"), ("nscores", "<i4"), ("n_acc", "<i4"),
                       ("n_candidates", "<i4"), ("best_acc_score", "<f4"), ("min_score_to_retain", "<f4")])
MEMBER_DTYPE = np.dtype([("kf_id", "<i4"), ("common_words", "<i4"), ("scored", "<i4"), ("si", "<f4")])
ACC_DTYPE = np.dtype([("acc_score", "<f4"), ("best_kf", "<i4")])
BRANCHES = ["empty_sharing", "excluded_hit", "excluded_not_live", "count_eq_min", "count_eq_min_plus1", "scored", "si_eq_minscore", "si_below_minscore",
            "empty_score_list", "neigh_not_live", "neigh_not_sharing", "neigh_excluded", "neigh_below_min_loop", "neigh_unscored_reloc",
            "neigh_unscored_nonzero", "neigh_better", "neigh_equal_score", "acc_eq_retain", "retained", "dropped", "dup_best", "same_first_word",
            "zero_weight", "best_is_start", "several_common"]
TWINS = dict(none=0, retain_ge=1, order_by_id=2, reloc_loop_gate=3, reversed_sum=4, reloc_not_persisted=5)

_oracle = None


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle():
    global _oracle
    if _oracle is None:
        d = tempfile.mkdtemp(prefix="kfdb_oracle_")
        so = os.path.join(d, "libkfdb_oracle.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "cpp", "kfdb_oracle.cpp")])
        L = C.CDLL(so)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.sd_kfdb_oracle_branches.restype = C.POINTER(C.c_int64)
        L.sd_kfdb_oracle_set_twin.argtypes = [i]
        L.sd_kfdb_oracle_new.restype = vp
        L.sd_kfdb_oracle_new.argtypes = [i]
        L.sd_kfdb_oracle_free.argtypes = [vp]
        L.sd_kfdb_oracle_clear.argtypes = [vp]
        L.sd_kfdb_oracle_add.argtypes = [vp, i, i, vp, vp]
        L.sd_kfdb_oracle_erase.argtypes = [vp, i]
        L.sd_kfdb_oracle_set_covisible.argtypes = [vp, i, i, vp]
        L.sd_kfdb_oracle_entry.argtypes = [vp, i, vp, vp, vp, vp]
        L.sd_kfdb_oracle_query.argtypes = [vp, i, i, i, vp, vp, f, i, vp, vp, vp, vp, vp]
        L.sd_kfdb_oracle_score.restype = f
        L.sd_kfdb_oracle_score.argtypes = [vp, i, vp, vp, i]
        L.sd_kfdb_oracle_l1.restype = C.c_double
        L.sd_kfdb_oracle_l1.argtypes = [i, vp, vp, i, vp, vp]
        assert L.sd_kfdb_oracle_branch_count() == len(BRANCHES)
        _oracle = L
    return _oracle


def bow(words, values):
    w = np.ascontiguousarray(words, U32).reshape(-1); v = np.ascontiguousarray(values, F64).reshape(-1)
    assert len(w) == len(v) and (len(w) < 2 or np.all(w[1:] > w[:-1]))
    return w, v


def _buf(a, dt):
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return a if len(a) else np.zeros(1, dt)


class OracleDB:
    def __init__(self, max_kf):
        self.L, self.n = oracle(), max_kf
        self.h = self.L.sd_kfdb_oracle_new(max_kf)

    def close(self):
        if self.h:
            self.L.sd_kfdb_oracle_free(self.h)
        self.h = None

    def add(self, kf, w, v):
        w, v = bow(w, v)
        return self.L.sd_kfdb_oracle_add(self.h, kf, len(w), _p(_buf(w, U32)), _p(_buf(v, F64)))

    def erase(self, kf):
        self.L.sd_kfdb_oracle_erase(self.h, kf)

    def clear(self):
        self.L.sd_kfdb_oracle_clear(self.h)

    def set_covisible(self, kf, neigh):
        nb = np.ascontiguousarray(neigh, I32).reshape(-1)
        self.L.sd_kfdb_oracle_set_covisible(self.h, kf, len(nb), _p(_buf(nb, I32)))

    def query(self, reloc, q, min_score=0.0, excluded=(), lane=0):
        w, v = bow(*q)
        ex = np.ascontiguousarray(excluded, I32).reshape(-1)
        info = np.zeros(1, INFO_DTYPE); mem = np.zeros(self.n, MEMBER_DTYPE); acc = np.zeros(self.n, ACC_DTYPE); cand = np.zeros(self.n, I32)
        self.L.sd_kfdb_oracle_query(self.h, lane, int(reloc), len(w), _p(_buf(w, U32)), _p(_buf(v, F64)), C.c_float(float(F32(min_score))), len(ex), _p(_buf(ex, I32)),
                                    _p(info), _p(mem), _p(acc), _p(cand))
        I = info[0]
        return dict(candidates=cand[:I["n_candidates"]].copy(), info=I.copy(), sharing=mem[:I["n_sharing"]].copy(), acc=acc[:I["n_acc"]].copy())

    def score(self, q, kf):
        w, v = bow(*q)
        return F32(self.L.sd_kfdb_oracle_score(self.h, len(w), _p(_buf(w, U32)), _p(_buf(v, F64)), int(kf)))

    def entry(self, kf):
        seq = C.c_uint32(); live = C.c_int(); rs = C.c_float(); n = C.c_int()
        self.L.sd_kfdb_oracle_entry(self.h, kf, C.byref(seq), C.byref(live), C.byref(rs), C.byref(n))
        return (int(seq.value), bool(live.value), F32(rs.value).tobytes())


def l1(a, b):
    """The oracle's L1Scoring::score as a double."""
    (w1, v1), (w2, v2) = bow(*a), bow(*b)
    return oracle().sd_kfdb_oracle_l1(len(w1), _p(_buf(w1, U32)), _p(_buf(v1, F64)), len(w2), _p(_buf(w2, U32)), _p(_buf(v2, F64)))


def branches():
    b = oracle().sd_kfdb_oracle_branches()
    return {name: int(b[i]) for i, name in enumerate(BRANCHES)}


def _ids_of(ops):
    return sorted({op[1] for op in ops if op[0] in ("add", "erase", "cov")})


def run_oracle(ops, max_kf, twin="none"):
    """The script through the sequential oracle, one query after the other -> (results, branches)."""
    L = oracle()
    L.sd_kfdb_oracle_reset_branches(); L.sd_kfdb_oracle_set_twin(TWINS[twin])
    db = OracleDB(max_kf)
    out = []
    try:
        for op in ops:
            if op[0] == "add":
                assert db.add(op[1], op[2], op[3]) == 0
            elif op[0] == "erase":
                db.erase(op[1])
            elif op[0] == "cov":
                db.set_covisible(op[1], op[2])
            elif op[0] == "clear":
                db.clear()
            elif op[0] == "loop":
                ex = op[3] or [()] * len(op[1])
                out.append([db.query(False, q, m, e) for q, m, e in zip(op[1], op[2], ex)])
            elif op[0] == "reloc":
                out.append([db.query(True, q) for q in op[1]])
            elif op[0] == "score":
                out.append([np.array([db.score(q, k) for k in ls], F32) for q, ls in zip(op[1], op[2])])
        out.append([db.entry(k) for k in _ids_of(ops)])
    finally:
        L.sd_kfdb_oracle_set_twin(0)
        db.close()
    return out, branches()


# ---------------------------------------------------------------- the numpy restatement (in its parallel terms)
def _si(q, e):
    qw, qv = q
    S = 0.0
    common, iq, ie = np.intersect1d(qw, e["word"], return_indices=True)
    for a, b in zip(iq, ie):                                    # ascending word order
        vi, wi = float(qv[a]), float(e["value"][b])
        S += (abs(vi - wi) - abs(vi)) - abs(wi)
    return common, F32(-S / 2.0)


class NumpyDB:
    def __init__(self, max_kf):
        self.e, self.seq = {}, 0

    def add(self, kf, w, v):
        assert kf not in self.e or not self.e[kf]["live"]
        w, v = bow(w, v)
        self.e[kf] = dict(word=w, value=v, seq=self.seq, live=True, reloc=F32(0.0), neigh=[])
        self.seq += 1

    def erase(self, kf):
        if kf in self.e:
            self.e[kf]["live"] = False

    def clear(self):
        self.e, self.seq = {}, 0

    def call(self, reloc, queries, min_scores=None, excluded=None):
        res, scored_by = [], []                                 # scored_by[q] = {kf: si} of the call's earlier queries
        for qi, q in enumerate(queries):
            q = bow(*q)
            ex = set(int(x) for x in (excluded[qi] if excluded else ()))
            share = []
            for kf, e in self.e.items():
                if not e["live"] or (not reloc and kf in ex):
                    continue
                common, si = _si(q, e)
                if len(common):
                    share.append((int(common[0]), e["seq"], kf, len(common), si))
            share.sort()
            start = F32(0.0) if reloc else F32(min_scores[qi])
            info = np.zeros(1, INFO_DTYPE)[0]
            info["best_acc_score"], info["min_score_to_retain"] = start, F32(0.75) * start
            rec = dict(candidates=np.zeros(0, I32), info=info, sharing=np.zeros(0, MEMBER_DTYPE), acc=np.zeros(0, ACC_DTYPE))
            scored_by.append({})
            res.append(rec)
            if not share:
                continue
            maxc = max(s[3] for s in share)
            minc = int(F32(maxc) * F32(0.8))
            count = {s[2]: s[3] for s in share}
            si_of = {s[2]: s[4] for s in share if s[3] > minc}
            scored_by[qi] = si_of
            rec["sharing"] = np.array([(kf, c, int(c > minc), si if c > minc else F32(0.0)) for _, _, kf, c, si in share], MEMBER_DTYPE)
            acc = []
            for _, _, kf, c, si in share:
                if not (c > minc and (reloc or si >= start)):
                    continue
                best, a, bk = si, si, kf
                for nb in self.e[kf]["neigh"]:
                    if nb not in self.e or not self.e[nb]["live"] or nb not in count:
                        continue
                    if reloc:
                        s2 = self.e[nb]["reloc"]
                        for p in range(qi, -1, -1):
                            if nb in scored_by[p]:
                                s2 = scored_by[p][nb]
                                break
                    else:
                        if nb not in si_of:
                            continue
                        s2 = si_of[nb]
                    a = F32(a + s2)
                    if s2 > best:
                        bk, best = nb, s2
                acc.append((a, bk))
            rec["acc"] = np.array(acc, ACC_DTYPE) if acc else np.zeros(0, ACC_DTYPE)
            bestacc = start
            for a, _ in acc:
                if a > bestacc:
                    bestacc = a
            retain = F32(0.75) * bestacc
            cand = []
            for a, bk in acc:
                if a > retain and bk not in cand:
                    cand.append(bk)
            rec["candidates"] = np.array(cand, I32)
            info["n_sharing"], info["max_common_words"], info["min_common_words"], info["nscores"] = len(share), maxc, minc, len(si_of)
            info["n_acc"], info["n_candidates"], info["best_acc_score"], info["min_score_to_retain"] = len(acc), len(cand), bestacc, retain
        if reloc:
            for qi in range(len(queries)):
                for kf, si in scored_by[qi].items():
                    self.e[kf]["reloc"] = si
        return res

    def score(self, q, kf):
        if kf not in self.e or not self.e[kf]["live"]:
            return F32(-1.0)
        return _si(bow(*q), self.e[kf])[1]


def run_numpy(ops, max_kf):
    db = NumpyDB(max_kf)
    out = []
    for op in ops:
        if op[0] == "add":
            db.add(op[1], op[2], op[3])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "cov":
            db.e[op[1]]["neigh"] = list(op[2])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "loop":
            out.append(db.call(False, op[1], op[2], op[3]))
        elif op[0] == "reloc":
            out.append(db.call(True, op[1]))
        elif op[0] == "score":
            out.append([np.array([db.score(q, k) for k in ls], F32) for q, ls in zip(op[1], op[2])])
    out.append([(db.e[k]["seq"], db.e[k]["live"], F32(db.e[k]["reloc"]).tobytes()) if k in db.e else (0, False, F32(0).tobytes()) for k in _ids_of(ops)])
    return out


# ---------------------------------------------------------------- the device
def run_device(fe, ops, max_kf, max_queries=8, max_query_words=None, pool_words=None, device=False):
    """The script through sd_kfdb_* (host CSR entry points; device=True: the device CSR ones).  One call per loop / reloc operation."""
    nq_words = [len(q[0]) for op in ops if op[0] in ("loop", "reloc", "score") for q in op[1]]
    pool = sum(len(op[2]) for op in ops if op[0] == "add")
    db = fe.KeyFrameDatabase(max_kf, pool_words or max(pool, 1), max(max_queries, 1), max_query_words or max(nq_words + [1]))
    out = []
    try:
        for op in ops:
            if op[0] == "add":
                db.add_host(op[1], op[2], op[3])
            elif op[0] == "erase":
                db.erase([op[1]])
            elif op[0] == "cov":
                db.set_covisible([op[1]], [op[2]])
            elif op[0] == "clear":
                db.clear()
            elif op[0] == "loop":
                out.append(db.detect_loop(op[1], op[2], op[3], device=device))
            elif op[0] == "reloc":
                out.append(db.detect_reloc(op[1], device=device))
            elif op[0] == "score":
                out.append(db.score(op[1], op[2]))
        ent = []
        for k in _ids_of(ops):
            e = db.entry(k)
            ent.append((e["seq"], e["live"], F32(e["reloc_score"]).tobytes()))
        out.append(ent)
    finally:
        db.close()
    return out


def assert_same(got, want, what=""):
    assert len(got) == len(want), "%s: %d vs %d results" % (what, len(got), len(want))
    for c, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        assert len(g) == len(w), "%s call %d: %d vs %d queries" % (what, c, len(g), len(w))
        for q, (a, b) in enumerate(zip(g, w)):
            if not isinstance(b, dict):
                assert np.asarray(a, F32).tobytes() == np.asarray(b, F32).tobytes(), "%s call %d query %d: scores %r vs %r" % (what, c, q, a, b)
                continue
            for key, dt in (("info", INFO_DTYPE), ("sharing", MEMBER_DTYPE), ("acc", ACC_DTYPE), ("candidates", I32)):
                x = np.ascontiguousarray(a[key], dt); y = np.ascontiguousarray(b[key], dt)
                assert x.tobytes() == y.tobytes(), "%s call %d query %d: %s differs\n got  %r\n want %r" % (what, c, q, key, x, y)
    assert list(got[-1]) == list(want[-1]), "%s: entries (seq, live, reloc_score) differ\n got  %r\n want %r" % (what, got[-1], want[-1])


def differs(a, b):
    try:
        assert_same(a, b)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------- crafted cases
def _up(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def _dn(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def case(name, max_kf, ops, claims, twin=None):
    return dict(name=name, max_kf=max_kf, ops=ops, claims=claims, twin=twin)


def case_min_score():
    """si ON min_score and one f32 step to either side; a second query for which nothing reaches min_score."""
    q = ([7], [1.0])
    ops = [("add", 0, [7], [0.25]), ("add", 1, [7], [_dn(0.25)]), ("add", 2, [7], [_up(0.25)]),
           ("loop", [q, q], [0.25, 0.5], None)]
    return case("min_score", 4, ops, ["si_eq_minscore", "si_below_minscore", "empty_score_list", "same_first_word"])


def case_retain(reloc):
    """acc ON 0.75f * best (1.0 beside 0.75) and one f32 step to either side."""
    q = ([1, 2, 3, 4], [1.0, 1.0, 1.0, 1.0])
    ops = [("add", 0, [1], [1.0]), ("add", 1, [2], [0.75]), ("add", 2, [3], [_up(0.75)]), ("add", 3, [4], [_dn(0.75)]),
           ("reloc", [q]) if reloc else ("loop", [q], [0.125], None)]
    return case("retain_%s" % ("reloc" if reloc else "loop"), 4, ops, ["acc_eq_retain", "retained", "dropped"], twin="retain_ge")


def case_min_common(maxc, reloc):
    """count ON minCommonWords = (int)(max * 0.8f), one above, one below; max in {1, 4, 5, 10, 15} -> 0, 3, 4, 8, 12."""
    minc = {1: 0, 4: 3, 5: 4, 10: 8, 15: 12}[maxc]
    words = list(range(10, 10 + maxc))
    q = (words, [2.0 ** -6] * maxc)
    ops, kf = [], 0
    for c in sorted({maxc, minc + 1, minc, minc - 1}):
        if c >= 1:
            ops.append(("add", kf, words[:c], [2.0 ** -7] * c)); kf += 1
    ops.append(("reloc", [q]) if reloc else ("loop", [q], [2.0 ** -9], None))
    claims = ["scored"] + (["count_eq_min", "count_eq_min_plus1", "several_common"] if maxc > 1 else [])
    return case("min_common_%d_%s" % (maxc, "reloc" if reloc else "loop"), 4, ops, claims)


def case_neighbour_scores(reloc):
    """A neighbour with an equal score does not replace pBestKF, a better one does, one equal to the new best does not."""
    q = ([1, 2, 3, 4], [1.0] * 4)
    ops = [("add", 0, [1], [0.5]), ("add", 1, [2], [0.5]), ("add", 2, [3], [0.75]), ("add", 3, [4], [0.75]),
           ("cov", 0, [1, 2, 3]), ("reloc", [q]) if reloc else ("loop", [q], [0.25], None)]
    return case("neighbour_scores_%s" % ("reloc" if reloc else "loop"), 4, ops, ["neigh_equal_score", "neigh_better"])


def case_zero_weight():
    """A shared word of weight zero: S = +0.0, si = -0.0f; not a reloc candidate (-0 > +0 is false), bestAccScore stays +0."""
    q = ([5], [0.5])
    ops = [("add", 0, [5], [0.0]), ("reloc", [q]), ("loop", [q], [0.0], None), ("score", [q], [[0, 1]])]
    return case("zero_weight", 2, ops, ["zero_weight", "best_is_start"])


def case_sum_order():
    """Three common words whose terms are -(2 + 2^-23), -2^-52, -2^-52: added in word order the small ones are lost (ties to even) and
    -S/2 = 1 + 2^-24 rounds to 1.0f; added from the back they survive and si = 1 + 2^-23."""
    v = [1.0 + 2.0 ** -24, 2.0 ** -53, 2.0 ** -53]
    q = ([3, 40, 500], v)
    ops = [("add", 0, [3, 40, 500], v), ("add", 1, [2, 3], [1.0, 0.875]), ("reloc", [q]), ("loop", [q], [0.5], None), ("score", [q], [[0]])]
    return case("sum_order", 2, ops, ["several_common"], twin="reversed_sum")


def case_list_order():
    """Ties on the first shared word go by sequence number, not by id -- also after erase and re-add; a smaller first shared word goes
    first whatever the sequence number; word ids above 2^31 order as unsigned."""
    hi = 0xFFFFFFF0
    q = ([4, 9, 0x80000005, hi], [1.0, 1.0, 1.0, 1.0])
    ops = [("add", 5, [9, hi], [0.5, 0.25]), ("add", 2, [9], [0.75]), ("add", 7, [9, 0x80000005], [0.5, 0.25]), ("add", 1, [0x80000005, hi], [0.5, 0.25]),
           ("add", 3, [hi], [0.75]), ("add", 6, [4], [0.75]),
           ("loop", [q], [0.125], None), ("reloc", [q]),
           ("erase", 5), ("add", 5, [9, hi], [0.5, 0.25]), ("loop", [q], [0.125], None), ("reloc", [q])]
    return case("list_order", 8, ops, ["same_first_word"], twin="order_by_id")


def case_excluded():
    """An excluded keyframe with the best score is nobody's neighbour and no candidate; an excluded id that is not live is ignored."""
    q = ([1, 2, 3], [1.0, 1.0, 1.0])
    ops = [("add", 0, [1], [0.5]), ("add", 1, [2], [1.0]), ("add", 2, [3], [0.5]), ("add", 3, [3], [0.5]), ("erase", 3),
           ("cov", 0, [1, 2]), ("cov", 2, [1]),
           ("loop", [q, q], [0.25, 0.25], [[1, 3, 6], []])]
    return case("excluded", 8, ops, ["excluded_hit", "excluded_not_live", "neigh_excluded", "neigh_not_sharing"])


def case_neighbour_not_live():
    """A neighbour that was erased, one that shares nothing with the query."""
    q = ([1, 2], [1.0, 1.0])
    ops = [("add", 0, [1], [0.5]), ("add", 1, [2], [1.0]), ("add", 2, [77], [1.0]), ("cov", 0, [1, 2]), ("erase", 1),
           ("loop", [q], [0.25], None), ("reloc", [q])]
    return case("neighbour_not_live", 4, ops, ["neigh_not_live", "neigh_not_sharing"])


def case_dup_best():
    """Three members name the same pBestKF: it is returned once, at its first position, before a later member's own."""
    q = ([1, 2, 3, 4], [1.0] * 4)
    ops = [("add", 0, [1], [0.25]), ("add", 3, [2], [1.0]), ("add", 1, [3], [1.0]), ("add", 2, [4], [0.25]),
           ("cov", 0, [1]), ("cov", 2, [1]), ("loop", [q], [0.25], None), ("reloc", [q])]
    return case("dup_best", 4, ops, ["dup_best", "neigh_better"])


def _reloc_entries():
    """A: five words, si 0.5 in q2; B: scored 0.5 by q1, shares one word with q2 (count 1 <= minCommonWords 4); C: five words, si 1.0."""
    a = ("add", 0, [10, 11, 12, 13, 14], [0.125, 0.125, 0.125, 0.0625, 0.0625])
    b = ("add", 1, [100], [0.5])
    c = ("add", 2, [20, 21, 22, 23, 24], [0.25, 0.25, 0.25, 0.125, 0.125])
    q1 = ([100], [0.5])
    q2 = ([10, 11, 12, 13, 14, 20, 21, 22, 23, 24, 100], [1.0] * 10 + [2.0 ** -20])
    return a, b, c, q1, q2


def case_reloc_two_calls():
    """Item 5 across two calls: q2 reads B's mRelocScore left by q1; with it A reaches 1.0 and is kept, without it A stays at 0.5."""
    a, b, c, q1, q2 = _reloc_entries()
    ops = [a, b, c, ("cov", 0, [1]), ("reloc", [q2]), ("reloc", [q1]), ("reloc", [q2])]
    return case("reloc_two_calls", 4, ops, ["neigh_unscored_reloc", "neigh_unscored_nonzero"], twin="reloc_not_persisted")


def case_reloc_one_call():
    """Item 5 inside one call: (q1, q2) as if run in order; (q2, q1) in a fresh state: q2 does not see the later q1."""
    a, b, c, q1, q2 = _reloc_entries()
    ops = [a, b, c, ("cov", 0, [1]), ("reloc", [q1, q2, q2]), ("clear",), a, b, c, ("cov", 0, [1]), ("reloc", [q2, q1])]
    return case("reloc_one_call", 4, ops, ["neigh_unscored_reloc", "neigh_unscored_nonzero"], twin="reloc_loop_gate")


def case_reloc_readd():
    """Item 5 after erase and re-add: the new entry's mRelocScore is +0 again (and it has no neighbours until they are set)."""
    a, b, c, q1, q2 = _reloc_entries()
    ops = [a, b, c, ("cov", 0, [1]), ("reloc", [q1]), ("erase", 1), b, ("reloc", [q2]), ("reloc", [q1, q2])]
    return case("reloc_readd", 4, ops, ["neigh_unscored_reloc", "neigh_unscored_nonzero"])


def case_loop_gate():
    """The loop form's neighbour gate: B is in the sharing list with a count <= minCommonWords and is not counted."""
    a, b, c, q1, q2 = _reloc_entries()
    ops = [a, b, c, ("cov", 0, [1]), ("loop", [q1], [0.25], None), ("loop", [q2], [0.25], None)]
    return case("loop_gate", 4, ops, ["neigh_below_min_loop"])


def case_empty():
    """A query that shares nothing, an empty query, an empty entry, an empty database."""
    q = ([1, 2], [0.5, 0.5])
    ops = [("loop", [q], [0.1], None), ("reloc", [q]), ("add", 0, [5], [1.0]), ("add", 1, [], []), ("loop", [q, ([], [])], [0.1, 0.1], None),
           ("reloc", [([], []), q]), ("score", [q, ([], [])], [[0, 1, 2], [1]])]
    return case("empty", 4, ops, ["empty_sharing"])


def crafted_cases():
    cs = [case_min_score(), case_zero_weight(), case_sum_order(), case_list_order(), case_excluded(), case_neighbour_not_live(), case_dup_best(),
          case_reloc_two_calls(), case_reloc_one_call(), case_reloc_readd(), case_loop_gate(), case_empty()]
    for reloc in (False, True):
        cs += [case_retain(reloc), case_neighbour_scores(reloc)]
        cs += [case_min_common(m, reloc) for m in (1, 4, 5, 10, 15)]
    return cs


# ---------------------------------------------------------------- seeded random scripts and shapes
def random_bow(rng, n_words, vocab):
    w = np.sort(rng.choice(vocab, size=min(n_words, vocab), replace=False)).astype(U32)
    v = rng.random(len(w)) + 1e-3
    return w, v / v.sum()


def random_script(seed, n_entries=300, max_kf=384, vocab=600, words=(1, 60), n_calls=6, queries_per_call=4):
    """Adds, erases and re-adds interleaved with neighbour updates and calls of both forms; values are arbitrary f64, so every score
    depends on the order of its sum."""
    rng = np.random.default_rng(seed)
    ops, live = [], []
    per_phase = n_entries // n_calls
    for phase in range(n_calls):
        for _ in range(per_phase):
            free = [k for k in range(max_kf) if k not in live]
            kf = int(rng.choice(free))
            ops.append(("add", kf) + random_bow(rng, int(rng.integers(words[0], words[1] + 1)), vocab)); live.append(kf)
            if len(live) > 8 and rng.random() < 0.15:
                gone = live.pop(int(rng.integers(len(live))))
                ops.append(("erase", gone))
        for kf in rng.choice(live, size=min(len(live), 40), replace=False):
            nb = [int(x) for x in rng.choice(max_kf, size=int(rng.integers(0, 11)), replace=False) if x != kf]
            ops.append(("cov", int(kf), nb))
        qs = [random_bow(rng, int(rng.integers(1, words[1] + 1)), vocab) for _ in range(queries_per_call)]
        if phase % 2 == 0:
            ex = [[int(x) for x in rng.choice(max_kf, size=int(rng.integers(0, 12)), replace=False)] for _ in qs]
            ops.append(("loop", qs, [float(F32(rng.random() * 0.02)) for _ in qs], ex))
            ops.append(("score", qs, [[int(x) for x in rng.integers(0, max_kf, size=7)] for _ in qs]))
        else:
            ops.append(("reloc", qs))
    return ops


def shape_script(n_entries, entry_words, query_words, shared="first", vocab_base=300000):
    """n_entries entries of entry_words words and one query of query_words words; an entry shares exactly one word with the query -- its
    first word (the query's first) or its last (the query's last) -- unless a size is 0.  Loop and reloc form and the scores."""
    qw = np.arange(query_words, dtype=np.int64) * 3 + vocab_base
    ops = []
    for k in range(n_entries):
        j = np.arange(max(entry_words - 1, 0), dtype=np.int64) + k % 5
        if not (entry_words and query_words):
            own = vocab_base + 1 + 3 * np.arange(entry_words, dtype=np.int64)                       # = 1 mod 3: never a query word
        elif shared == "first":
            own = np.concatenate([[qw[0]], qw[0] + 1 + 3 * j])
        else:
            own = np.concatenate([(qw[-1] - 2 - 3 * j)[::-1], [qw[-1]]])
        v = (np.arange(len(own)) % 5 + 1) * 2.0 ** -12
        ops.append(("add", k, own.astype(U32), v))
    q = (qw.astype(U32), (np.arange(query_words) % 7 + 1) * 2.0 ** -13)
    for k in range(0, n_entries, 3):
        ops.append(("cov", k, [(k + 1) % n_entries, (k + 2) % n_entries]))
    ops += [("loop", [q], [2.0 ** -14], None), ("reloc", [q]), ("score", [q], [list(range(min(n_entries, 5)))])]
    return ops
