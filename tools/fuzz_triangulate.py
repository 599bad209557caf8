"""Randomised parity sweep of sd_batch_search_for_triangulation / sd_batch_create_new_map_points against the sequential CPU oracle
(developer tool): synthetic two-view scenes of random size, neighbour count, mono share, pixel noise, level count and baseline rule;
every match array, pair list and sd_new_map_point record byte for byte."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
import triangulate_cases as tc


def run(n_cases, seed0):
    pkg = g.load_package(); orc = g.load_oracle()
    fe, synth = pkg.frontend, pkg.synth
    rng = np.random.default_rng(seed0)
    voc = tc.vocabulary(synth, 5)
    O = orc.Vocabulary.from_nodes(voc)
    stats = dict(pairs=0, matches=0, new=0)
    for nlevels in (8, 12):
        ws = tc.Workspace(fe, 24, voc, dict(tc.GEOM, nlevels=nlevels))
        try:
            for k in range(n_cases):
                n = int(rng.integers(1, min(ws.cap, 400))); nb = int(rng.integers(0, 21)); median = bool(rng.integers(0, 2))
                c = tc.random_scene(voc, 1000 * seed0 + k, n, nb, mono_share=float(rng.choice([0.0, 0.4, 1.0])), noise=float(rng.choice([0.0, 0.5, 2.0])),
                                    lv=ws.lv, median=median)
                kfs = [c["kf1"]] + c["neighbours"]
                tc.attach_bow(kfs, O)
                ws.upload(kfs)
                hk = ws.has_table([c["kf1"]]); hn = ws.has_table(c["neighbours"]) if nb else None
                ws.b.create_new_map_points([0], [c["kf1"]["Tcw"]], [0, nb], list(range(1, nb + 1)), [x["Tcw"] for x in c["neighbours"]] or np.zeros((0, 16), np.float32),
                                           tc.CAM, neigh_median_depth=c["median_depth"], d_kf_has_mp=hk.data_ptr() if hk is not None else None,
                                           d_neigh_has_mp=hn.data_ptr() if hn is not None else None)
                o = tc.create(c["kf1"], c["neighbours"], c["median_depth"], lv=ws.lv)["new"]
                what = None if ws.b.download_new_map_points(0).tobytes() == o.tobytes() else "create_new_map_points"
                stats["new"] += len(o)
                if what is None and nb:
                    only, ori = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                    h1 = ws.has_table([c["kf1"]] * nb)
                    ws.b.search_for_triangulation([0] * nb, list(range(1, nb + 1)), [c["kf1"]["Tcw"]] * nb, [x["Tcw"] for x in c["neighbours"]], tc.CAM,
                                                  d_has_mp1=h1.data_ptr() if h1 is not None else None, d_has_mp2=hn.data_ptr() if hn is not None else None,
                                                  only_stereo=only, checkOrientation=ori)
                    for p in range(nb):
                        r = tc.search(c["kf1"], c["neighbours"][p], lv=ws.lv, only_stereo=only, check_orientation=ori)
                        m, pr, nm = ws.b.download_matches(p)
                        stats["pairs"] += 1; stats["matches"] += nm
                        if nm != r["nmatches"] or not np.array_equal(m[:n], r["match"]) or pr.tobytes() != r["pairs"].tobytes():
                            what = "search_for_triangulation pair %d (%d vs %d)" % (p, nm, r["nmatches"])
                            break
                if what is not None:
                    print("MISMATCH levels %d case %d (%s): %s" % (nlevels, k, c["name"], what))
                    return 1
        finally:
            ws.close()
    print("fuzz_triangulate: %d cases identical" % (2 * n_cases), stats)
    return 0


if __name__ == "__main__":
    sys.exit(run(int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 3))
