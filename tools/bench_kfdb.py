"""Timing of the device KeyFrameDatabase queries (k_kfdb.h), written to profiles/kfdb_bench.json and printed as ONE JSON line.
`--entries` keyframes of about `--words` words over a word-id space of `--space`, eight to a place (a keyframe or a query holds 85 % of its
place's words and 15 % of its own) with its ten nearest ids as covisibility neighbours; calls of 1, 16 and 64 queries.  Per size and form:
  device_call_ms     a host clock around `--calls` calls of sd_kfdb_detect_loop / _reloc (device CSR, arrays already in HBM) that end in one
                     device synchronise, after warm-up: the cost of a call in a stream of calls
  device_latency_ms  the same with every call followed by sd_kfdb_download_candidates of its first query (one synchronise and two small
                     copies): what a caller waits for one answer
  oracle_ms          the sequential CPU oracle (tests/cpp/kfdb_oracle.cpp: the inverted file of lists) on the same queries, one after the
                     other on 1 host thread and, loop form only, spread over 16 host threads (one set of marks per thread; the reloc form
                     writes mRelocScore and stays on one thread), wall clock, median of three
Results are compared byte for byte inside the run.  No ratio is required: the device matches every query against every entry, the
inverted file walks only the lists of the query's words, and at one query the host may well be faster."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import kfdb_cases as kc  # noqa: E402


def make_bow(rng, n, space, base=None):
    w = np.unique(rng.integers(0, space, n))
    if base is not None:                                         # 85 % of the place's words, the rest its own
        w = np.unique(np.concatenate([w[:int(0.15 * len(w))], rng.choice(base, int(0.85 * len(base)), replace=False)]))
    v = rng.random(len(w)) + 1e-3
    return w.astype(np.uint32), v / v.sum()


def median3(fn):
    ts, out = [], None
    for _ in range(3):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(sorted(ts)[1], 3), out


def same(a, b):
    return all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a, b) for k in ("candidates", "info", "sharing", "acc")) and len(a) == len(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=4096)
    ap.add_argument("--words", type=int, default=1500)
    ap.add_argument("--space", type=int, default=1000000)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_bench.json"))
    a = ap.parse_args()
    import torch
    fe = g.load_package().frontend
    if fe.device_count() < 1:
        raise SystemExit("bench_kfdb needs a HIP device")
    L = fe.lib()
    rng = np.random.default_rng(7)
    N, maxq = a.entries, max(a.queries)
    places = [make_bow(rng, a.words, a.space)[0] for _ in range((N + 7) // 8)]
    entries = [make_bow(rng, a.words, a.space, places[k // 8]) for k in range(N)]
    neigh = [[(k + d) % N for d in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5)] for k in range(N)]
    queries = [make_bow(rng, a.words, a.space, places[int(rng.integers(len(places)))]) for _ in range(maxq)]
    excluded = [[int(x) for x in rng.choice(N, 20, replace=False)] for _ in range(maxq)]
    min_score = [0.01] * maxq
    db = fe.KeyFrameDatabase(N, sum(len(w) for w, _ in entries), maxq, max(len(w) for w, _ in queries))
    odb = kc.OracleDB(N)
    rec = dict(tool="bench_kfdb", entries=N, words_per_entry=int(np.mean([len(w) for w, _ in entries])), word_space=a.space, timed_calls=a.calls,
               host_cpus=len(os.sched_getaffinity(0)), sizes=[])
    try:
        for k, (w, v) in enumerate(entries):
            db.add_host(k, w, v); odb.add(k, w, v)
        db.set_covisible(list(range(N)), neigh)
        for k in range(N):
            odb.set_covisible(k, neigh[k])
        for nq in a.queries:
            qs = queries[:nq]
            off, qw, qv = fe.pack_bow_queries(qs)
            eo, ei = fe._pack_ids(excluded[:nq], nq)
            ms = np.array(min_score[:nq], np.float32)
            d_w = torch.from_numpy(qw.view(np.int32).copy()).cuda(); d_v = torch.from_numpy(qv.copy()).cuda()
            torch.cuda.synchronize()
            pw, pv = C.c_void_p(d_w.data_ptr()), C.c_void_p(d_v.data_ptr())
            info = np.zeros(1, fe.KFDB_INFO_DTYPE); cand = np.zeros(N, np.int32)
            forms = dict(loop=lambda: fe.check(L.sd_kfdb_detect_loop(db.h, nq, kc._p(off), pw, pv, kc._p(ms), kc._p(eo), kc._p(ei), None)),
                         reloc=lambda: fe.check(L.sd_kfdb_detect_reloc(db.h, nq, kc._p(off), pw, pv, None)))
            fetch = lambda: fe.check(L.sd_kfdb_download_candidates(db.h, 0, kc._p(cand), N, kc._p(info), None, 0, None, 0))
            size = dict(queries=nq)
            for form, call in forms.items():
                for _ in range(a.warmup):
                    call()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.calls):
                    call()
                torch.cuda.synchronize()
                call_ms = (time.perf_counter() - t) * 1e3 / a.calls
                t = time.perf_counter()
                for _ in range(a.calls):
                    call(); fetch()
                lat_ms = (time.perf_counter() - t) * 1e3 / a.calls
                size[form] = dict(device_call_ms=round(call_ms, 4), device_latency_ms=round(lat_ms, 4))
            got = db.detect_loop(qs, ms, excluded[:nq], device=True)
            o1, ref = median3(lambda: [odb.query(False, q, m, e) for q, m, e in zip(qs, ms, excluded[:nq])])
            tl = threading.local(); lanes = iter(range(16)); lk = threading.Lock()

            def task(i):
                if not hasattr(tl, "lane"):
                    with lk:
                        tl.lane = next(lanes)
                return odb.query(False, qs[i], ms[i], excluded[i], lane=tl.lane)

            with ThreadPoolExecutor(16) as pool:
                o16, ref16 = median3(lambda: list(pool.map(task, range(nq))))
            size["loop"].update(oracle_ms_1_thread=o1, oracle_ms_16_threads=o16, identical_to_oracle=bool(same(got, ref) and same(ref16, ref)),
                                candidates=int(sum(len(r["candidates"]) for r in ref)), scored=int(sum(r["info"]["nscores"] for r in ref)))
            # mRelocScore after a call is the score of the last query that scored the entry, whatever it was before: once the oracle has
            # run the call's queries too, both sides hold the same members, and every further pass reads and leaves them unchanged
            for q in qs:
                odb.query(True, q)
            got = db.detect_reloc(qs, device=True)
            o1r, refr = median3(lambda: [odb.query(True, q) for q in qs])
            size["reloc"].update(oracle_ms_1_thread=o1r, identical_to_oracle=bool(same(got, refr)),
                                 candidates=int(sum(len(r["candidates"]) for r in refr)), scored=int(sum(r["info"]["nscores"] for r in refr)))
            for form in ("loop", "reloc"):
                size[form]["oracle_1_thread_over_device_latency"] = round(size[form]["oracle_ms_1_thread"] / size[form]["device_latency_ms"], 2)
            rec["sizes"].append(size)
    finally:
        db.close(); odb.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
