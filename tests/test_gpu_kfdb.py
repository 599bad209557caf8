"""GPU parity of the device KeyFrameDatabase (sd_kfdb_*) with the sequential CPU oracle (tests/cpp/kfdb_oracle.cpp), byte for byte:
candidates, their order, every count and every f32 of the intermediate record.  The crafted cases of kfdb_cases.py, the shapes at which
the kernels take another path, the independence of a query from its call, the path from extracted frames, the refusals and seeded
random databases."""
import numpy as np
import pytest

import kfdb_cases as kc
import triangulate_cases as tc

pytestmark = pytest.mark.gpu
CASES = kc.crafted_cases()


def check(fe, ops, max_kf, what, **kw):
    want, _ = kc.run_oracle(ops, max_kf)
    got = kc.run_device(fe, ops, max_kf, **kw)
    kc.assert_same(got, want, what)
    return want


def test_records_are_the_headers(gpu, fe):
    assert fe.KFDB_INFO_DTYPE == kc.INFO_DTYPE and fe.KFDB_MEMBER_DTYPE == kc.MEMBER_DTYPE and fe.KFDB_ACC_DTYPE == kc.ACC_DTYPE
    assert kc.INFO_DTYPE.itemsize == 32 and kc.MEMBER_DTYPE.itemsize == 16 and kc.ACC_DTYPE.itemsize == 8


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_cases(gpu, fe, case):
    check(fe, case["ops"], case["max_kf"], case["name"])
    check(fe, case["ops"], case["max_kf"], case["name"] + " (device CSR)", device=True)


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("n_entries", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_entry_counts(gpu, fe, n_entries):
    """Around the 4 entries of a match workgroup, the 64 lanes of a wave, the 256 threads of the threshold kernel and the 1024 of the
    per-query tail."""
    want = check(fe, kc.shape_script(n_entries, 65, 64), max(n_entries, 1), "%d entries" % n_entries)
    assert want[0][0]["info"]["n_sharing"] == n_entries


@pytest.mark.parametrize("shared", ["first", "last"])
@pytest.mark.parametrize("words", [0, 1, 63, 64, 65, 255, 256, 257, 3000])
def test_entry_and_query_lengths(gpu, fe, words, shared):
    """Entries and queries of 0 .. a few thousand words (64 lanes x 4 searches in flight = 256 words per step), the only shared word
    first or last in the entry."""
    want = check(fe, kc.shape_script(5, words, 65, shared), 5, "entries of %d words" % words)
    assert want[0][0]["info"]["n_sharing"] == (5 if words else 0)
    want = check(fe, kc.shape_script(5, 65, words, shared), 5, "query of %d words" % words)
    assert want[0][0]["info"]["n_sharing"] == (5 if words else 0)


def test_query_at_max_query_words(gpu, fe):
    """A query of exactly max_query_words = SD_KFDB_MAX_QUERY_WORDS words (the whole 64 KB of LDS the match kernel may ask for); one word
    more is refused."""
    n = fe.KFDB_MAX_QUERY_WORDS
    ops = kc.shape_script(3, 40, n, "last")
    want = check(fe, ops, 3, "query at the maximum", max_query_words=n)
    assert want[0][0]["info"]["n_sharing"] == 3
    db = fe.KeyFrameDatabase(4, 64, 1, 100)
    try:
        q = (np.arange(101, dtype=np.uint32), np.ones(101))
        with pytest.raises(fe.SdError) as e:
            db.detect_reloc([q])
        assert e.value.code == fe.SD_ERR_CAPACITY
        db.detect_reloc([(q[0][:100], q[1][:100])])
    finally:
        db.close()
    with pytest.raises(fe.SdError) as e:
        fe.KeyFrameDatabase(4, 64, 1, n + 1)
    assert e.value.code == fe.SD_ERR_INVALID


@pytest.mark.parametrize("n", [4096, 4097])
def test_sharing_list_at_and_over_the_lds_sort(gpu, fe, n):
    """4096 members are ordered in LDS, 4097 in the database's scratch rows: all share the query's only word, so the order is the
    sequence numbers' -- ids are added in a shuffled order -- and every member is kept."""
    rng = np.random.default_rng(n)
    ids = rng.permutation(n + 3)[:n]
    ops = [("add", int(k), [9, 10 + int(k)], [2.0 ** -3, 2.0 ** -4]) for k in ids]
    ops += [("loop",[([9], [2.0 ** -4])], [2.0 ** -5], None), ("reloc", [([9], [2.0 ** -4])])]
    want = check(fe, ops, n + 3, "%d members" % n, max_queries=1)
    assert list(want[0][0]["sharing"]["kf_id"]) == [int(k) for k in ids] and want[0][0]["info"]["n_candidates"] == n


# ---------------------------------------------------------------- independence
def test_a_query_does_not_depend_on_its_call(gpu, fe):
    """Loop form and score: three queries in one call give the records they give alone (the reloc form differs by mRelocScore only:
    kfdb_cases.case_reloc_one_call)."""
    ops = kc.random_script(11, n_entries=120, max_kf=160, vocab=200, words=(1, 40), n_calls=1, queries_per_call=3)
    base = [op for op in ops if op[0] in ("add", "erase", "cov")]
    call = [op for op in ops if op[0] == "loop"][0]
    sc = [op for op in ops if op[0] == "score"][0]
    together = kc.run_device(fe, base + [call, sc], 160)
    for q in range(3):
        alone = kc.run_device(fe, base + [("loop", [call[1][q]], [call[2][q]], [call[3][q]]), ("score", [sc[1][q]], [sc[2][q]])], 160)
        kc.assert_same([[together[0][q]], [together[1][q]], together[2]], alone, "query %d alone" % q)
    want, _ = kc.run_oracle(base + [call, sc], 160)
    kc.assert_same(together, want, "together")


# ---------------------------------------------------------------- from extracted frames
def test_frames_through_extract_bow_add_and_query(gpu, fe, orc, synth):
    """Synthetic frames -> ORB -> ComputeBoW -> add_from_batch (device to device); queries are other slots of the batch; the oracle is
    fed by download_bow."""
    cfg = synth.KITTI_STEREO
    T = 6
    ex = fe.ORBextractor(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["ini_th_fast"], cfg["min_th_fast"])
    b = fe.Batch(ex, cfg["width"], cfg["height"], T)
    V = fe.Vocabulary.from_nodes(tc.vocabulary(synth, 5))
    db = fe.KeyFrameDatabase(16, 8 * b.cap, 4, b.cap)
    try:
        b.extract_host(np.stack([synth.stereo_frame(seq=4, t=t)[0] for t in range(T)]))
        with pytest.raises(fe.SdError) as e:
            db.add(b, [0], [3])                                   # no bag of words yet
        assert e.value.code == fe.SD_ERR_STATE
        with pytest.raises(fe.SdError) as e:
            db.detect_reloc([0], batch=b)
        assert e.value.code == fe.SD_ERR_STATE
        b.compute_bow(V, list(range(T)), 4)
        kf_of = {0: 7, 1: 2, 2: 11, 3: 5}
        db.add(b, list(kf_of), list(kf_of.values()))
        bows = [b.download_bow(t) for t in range(T)]
        assert min(len(x["word"]) for x in bows) > 50
        db.set_covisible([7, 2, 11], [[2, 11], [7], [5, 9]])
        ops = [("add", kf_of[t], bows[t]["word"], bows[t]["value"]) for t in kf_of]
        ops += [("cov", 7, [2, 11]), ("cov", 2, [7]), ("cov", 11, [5, 9])]
        qs = [(bows[t]["word"], bows[t]["value"]) for t in (4, 5, 0)]
        ops += [("loop", qs, [0.01, 0.05, 0.01], [[], [2], [7]]), ("reloc", qs)]
        want, _ = kc.run_oracle(ops, 16)
        got = [db.detect_loop([4, 5, 0], [0.01, 0.05, 0.01], [[], [2], [7]], batch=b), db.detect_reloc([4, 5, 0], batch=b)]
        ent = []
        for k in sorted(kf_of.values()):
            en = db.entry(k)
            t = [s for s in kf_of if kf_of[s] == k][0]
            assert en["word"].tobytes() == bows[t]["word"].tobytes() and en["value"].tobytes() == bows[t]["value"].tobytes()
            ent.append((en["seq"], en["live"], np.float32(en["reloc_score"]).tobytes()))
        kc.assert_same(got + [ent], want, "frames")
        assert want[0][0]["info"]["n_sharing"] == 4 and want[0][2]["info"]["n_sharing"] == 3 and want[1][2]["info"]["n_candidates"] >= 1
    finally:
        db.close(); V.close(); b.close()


# ---------------------------------------------------------------- refusals
def test_refusals(gpu, fe):
    db = fe.KeyFrameDatabase(4, 10, 2, 8)
    try:
        db.add_host(1, [1, 2, 3], [0.5, 0.25, 0.25])
        for bad, code in ((lambda: db.add_host(1, [4], [1.0]), fe.SD_ERR_STATE),                       # live id added again
                          (lambda: db.add_host(2, [3, 3], [0.5, 0.5]), fe.SD_ERR_INVALID),             # words not strictly ascending
                          (lambda: db.add_host(2, [4, 3], [0.5, 0.5]), fe.SD_ERR_INVALID),
                          (lambda: db.add_host(4, [4], [1.0]), fe.SD_ERR_INVALID),                     # id outside [0, max_keyframes)
                          (lambda: db.add_host(2, np.arange(8), np.ones(8)), fe.SD_ERR_CAPACITY),      # 3 + 8 > 10 pool words
                          (lambda: db.set_covisible([2], [[1]]), fe.SD_ERR_STATE),                     # not in the database
                          (lambda: db.set_covisible([1], [[7]]), fe.SD_ERR_INVALID),
                          (lambda: db.set_covisible([1], [list(range(11))]), fe.SD_ERR_INVALID),
                          (lambda: db.detect_reloc([([1], [1.0])] * 3), fe.SD_ERR_CAPACITY),           # three queries, max_queries = 2
                          (lambda: db.detect_reloc([(np.arange(9), np.ones(9))]), fe.SD_ERR_CAPACITY),
                          (lambda: db.detect_loop([([1], [1.0])], 0.1, [[4]]), fe.SD_ERR_INVALID),     # excluded id out of range
                          (lambda: db.score([([1], [1.0])], [[-1]]), fe.SD_ERR_INVALID)):
            with pytest.raises(fe.SdError) as e:
                bad()
            assert e.value.code == code
        assert fe.lib().sd_kfdb_download_candidates(db.h, 0, None, 0, None, None, 0, None, 0) == fe.SD_ERR_STATE      # no query has run
        r = db.detect_reloc([([2], [0.25])])
        assert list(r[0]["candidates"]) == [1]                   # the refused calls left the database as it was
        e1 = db.entry(1)
        assert e1["live"] and e1["seq"] == 0 and list(e1["word"]) == [1, 2, 3] and e1["reloc_score"] == np.float32(0.25)
        db.erase([1]); db.add_host(1, [2], [0.5])               # the pool is not reclaimed: 3 + 1 words used
        with pytest.raises(fe.SdError) as e:
            db.add_host(2, np.arange(7), np.ones(7))
        assert e.value.code == fe.SD_ERR_CAPACITY
        assert db.entry(1)["seq"] == 1 and db.entry(1)["reloc_score"].tobytes() == np.float32(0.0).tobytes()
        db.clear()
        assert not db.entry(1)["live"]
        db.add_host(2, np.arange(8), np.ones(8))
        assert db.entry(2)["seq"] == 0
    finally:
        db.close()


# ---------------------------------------------------------------- random databases
@pytest.mark.parametrize("seed", range(8))
def test_random_databases(gpu, fe, seed):
    """About 300 entries with add / erase / re-add interleaved, neighbours, both forms in calls of four queries, scores of listed ids."""
    ops = kc.random_script(100 + seed)
    want, br = kc.run_oracle(ops, 384)
    got = kc.run_device(fe, ops, 384, device=bool(seed & 1))
    kc.assert_same(got, want, "seed %d" % seed)
    assert br["neigh_better"] > 0 and br["neigh_unscored_reloc"] > 0
