"""The crafted frame pair of area_cases.py reaches every seam it is meant to pin: the column spans, hit counts, ties and clipped
borders are computed here in numpy from the camera and the radius alone, so the generator cannot silently miss one; the CPU oracle
then finds what the dense windows were built to yield.  No GPU."""
import numpy as np
import pytest

import area_cases as ac
import triangulate_cases as tc


@pytest.fixture(scope="module")
def sc():
    return ac.scene()


@pytest.fixture(scope="module")
def scale():
    return tc.Levels().scale


def test_size_and_domain(sc):
    for f in (sc["last"], sc["cur"]):
        k = f["kp"]
        assert len(k) <= 300 and f["desc"].shape == (len(k), 32)
        assert ((k["x"] >= 0) & (k["x"] < ac.W) & (k["y"] >= 0) & (k["y"] < ac.H)).all()
    px, py = ac.cells(sc["cur"]["kp"])
    assert ((px >= 0) & (px < ac.COLS) & (py >= 0) & (py < ac.ROWS)).all(), "every current key point lies in the grid"
    u, v = ac.project(sc["xw"])
    assert ((u >= 0) & (u <= ac.W) & (v >= 0) & (v <= ac.H)).all()


def test_windows_share_no_member(sc, scale):
    """Windows with different centres are disjoint: what a window holds is what was placed for it."""
    P, L = ac.proj_windows(sc, scale), ac.local_windows(sc, scale)
    owner = {}
    for name, w in list(P.items()) + list(L.items()):
        key = name.split("_", 1)[1] if name.startswith(("distinct_", "tied_")) else name
        for i in w["order"]:
            assert owner.setdefault(int(i), key) == key, "key point %d lies in the windows of %s and %s" % (i, owner[int(i)], key)
    assert len(owner) == len(sc["cur"]["kp"]), "every current key point belongs to a window"


def test_search_by_projection_seams_occur(sc, scale):
    P = ac.proj_windows(sc, scale)
    assert {P["span_16"]["span"], P["span_17"]["span"]} == {16, 17}
    for name in ("span_16", "span_17"):
        w = P[name]
        assert w["cols"][0] == w["first_col"] and w["cols"][-1] == w["last_col"], "%s: members in the first and the last column" % name
        assert 0 < len(w["hits"]) <= 16 and w["outside"] >= 2 and not w["clipped"]
    for n in (16, 17, 64, 65):
        d, t = P["distinct_%d" % n], P["tied_%d" % n]
        assert d["span"] <= 16 and not d["clipped"], "only the hit count may send the point to the whole wave"
        assert len(d["hits"]) == len(t["hits"]) == n == len(d["order"])
        assert len(set(d["dist"])) == n and list(d["dist"]) == list(range(n - 1, -1, -1)), "each member visited later is nearer"
        assert set(t["dist"]) == {63, 64} and min(np.bincount(t["dist"])[63:]) >= n // 2
    for side in ("left", "right", "top", "bottom"):
        w = P["clip_" + side]
        assert w["clipped"] == {side} and len(w["hits"]) == 3


def test_search_local_map_seams_occur(sc, scale):
    L = ac.local_windows(sc, scale)
    assert [len(L["distinct_%d" % n]["hits"]) for n in (64, 65)] == [64, 65], "overflow flag 0 and 1"
    assert [len(L["tied_%d" % n]["hits"]) for n in (64, 65)] == [64, 65]
    assert list(L["distinct_65"]["dist"]) == list(range(64, -1, -1)) and set(L["tied_65"]["dist"]) == {63, 64}
    assert L["clip_corner"]["clipped"] == {"left", "top"} and len(L["clip_corner"]["hits"]) == 3


def test_the_oracle_finds_what_the_dense_windows_hold(sc, scale, orc):
    """The nearest member of a `distinct` point is the last one visited: position 64 of 65 lies beyond the 64-key row."""
    cur, last = sc["cur"], sc["last"]
    P, L = ac.proj_windows(sc, scale), ac.local_windows(sc, scale)
    om, opairs, onm = orc.search_by_projection(cur["kp"], cur["desc"], cur["ur"], last["kp"], last["desc"], sc["xw"], sc["flags"], ac.IDENTITY,
                                               ac.IDENTITY, ac.cam_array(), scale, ac.TH_PROJ, False, True)
    names = [n for n, _ in sc["proj"]]
    assert onm == len(names), "every last-frame point finds a match"
    for n in (16, 17, 64, 65):
        assert om[P["distinct_%d" % n]["hits"][-1]] == names.index("distinct_%d" % n)
    pts = np.ascontiguousarray(sc["points"]).view(orc.MAP_POINT_DTYPE)
    otr, opm, okm, onm = orc.search_local_map(cur["kp"], cur["desc"], cur["ur"], pts, sc["pdesc"], ac.IDENTITY, ac.cam_array(), scale, ac.TH_LOCAL,
                                              0.8, 0.5)
    assert otr["in_view"].all() and (otr["level"] == 0).all() and (otr["view_cos"] > 0.998).all()
    for n in (64, 65):
        assert opm[sc["local"].index("distinct_%d" % n)] == L["distinct_%d" % n]["hits"][-1]
    assert opm[sc["local"].index("clip_corner")] >= 0
