"""GPU: every crafted image of tests/extract_cases.py on the device against the oracle, byte for byte: pyramid and blurred planes of
every level, FAST candidate counts, per-level counts, key points and descriptors.  Images of one size and one extractor setting
share a Batch (the largest holds more than 8 images: the staged FAST kernel's image order blockIdx.y * 8 + (blockIdx.x & 7) then has
a partly filled last group).  tests/test_extract_cases.py says, on the CPU, what each named case reaches."""
import importlib.util
import os

import numpy as np
import pytest

import extract_cases as E
from conftest import assert_kp_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shots(orc):
    return E.build_all(orc)


_oracle = {}


def oracle_run(orc, shot):
    """The oracle's outputs of one shot, computed once and shared."""
    if shot.name not in _oracle:
        o = orc.Extractor(*shot.params)
        kp, desc = o(shot.img)
        nl = shot.params[2]
        _oracle[shot.name] = (kp, desc, o.per_level.copy(), o.cand_per_level.copy(), [o.pyramid(l) for l in range(nl)], [o.blurred(l) for l in range(nl)])
    return _oracle[shot.name]


def named(shot):
    names = [c.name for c in shot.cases]
    return "%s [%s%s]" % (shot.name, "; ".join(names[:8]), "; ... %d more" % (len(names) - 8) if len(names) > 8 else "")


def groups(shots):
    g = {}
    for s in shots:
        g.setdefault((s.img.shape, s.params), []).append(s)
    return g


def run_group(fe, orc, group, order=None):
    """One Batch over the group's images (in `order`); returns the device bytes per shot name after comparing everything with the oracle."""
    order = list(range(len(group))) if order is None else order
    (h, w), prm = group[0].img.shape, group[0].params
    ex = fe.ORBextractor(*prm)
    b = fe.Batch(ex, w, h, len(order))                   # an unsupported geometry raises SdError: a failure of the crafted size, not a skip
    b.extract_host(np.stack([group[k].img for k in order]))
    out = {}
    try:
        for slot, k in enumerate(order):
            s = group[k]
            rk, rd, per_level, cand, pyr, blur = oracle_run(orc, s)
            what = "%s, slot %d of %d" % (named(s), slot, len(order))
            for l in range(prm[2]):
                assert np.array_equal(b.pyramid(slot, l), pyr[l]), "pyramid level %d: %s" % (l, what)
                assert np.array_equal(b.blurred(slot, l), blur[l]), "blurred level %d: %s" % (l, what)
            got = b.candidate_counts(slot)
            assert np.array_equal(got, cand), "FAST candidate counts %r vs %r: %s" % (got, cand, what)
            kp, desc, pl = b.download(slot)
            assert np.array_equal(pl, per_level), "per-level counts %r vs %r: %s" % (pl, per_level, what)
            assert_kp_equal(kp, rk, what)
            assert kp.tobytes() == rk.tobytes(), "key point bytes: %s" % what
            assert np.array_equal(desc, rd), "descriptors: %s" % what
            out[s.name] = (kp.tobytes(), desc.tobytes())
    finally:
        b.close()
    return out


@pytest.mark.parametrize("builder", E.BUILDERS)
def test_crafted_images_match_oracle(gpu, fe, orc, shots, builder):
    gs = groups(shots[builder])
    for group in gs.values():
        run_group(fe, orc, group)
    if builder == "threshold_edges":
        assert max(len(g) for g in gs.values()) >= 9 and any(len(g) % 8 for g in gs.values() if len(g) > 8)


@pytest.mark.parametrize("builder", ["threshold_edges", "nms_ties", "retry", "lattice", "planes"])
def test_alone_and_in_another_slot(gpu, fe, orc, shots, builder):
    """A named image gives the same bytes alone, in its group, and in the group reversed (another slot, other neighbours)."""
    group = max(groups(shots[builder]).values(), key=len)
    if len(group) < 2:                                   # a lone image gets its point reflection for company
        group = group + [E.Shot(group[0].name + "/reflected", np.ascontiguousarray(group[0].img[::-1, ::-1]), group[0].params, [])]
    full = run_group(fe, orc, group)
    rev = run_group(fe, orc, group, order=list(range(len(group)))[::-1])
    for k in (0, len(group) - 1):
        alone = run_group(fe, orc, group, order=[k])
        assert alone[group[k].name] == full[group[k].name] == rev[group[k].name], named(group[k])


def test_crafted_fuzz_draws(gpu, capsys):
    """8 fixed --crafted draws of tools/fuzz_extract.py (lattices, sparse dots, plateaus; nfeatures down to 1): identical to the oracle."""
    spec = importlib.util.spec_from_file_location("fuzz_extract", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_extract.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    assert m.run(E.FUZZ_DRAWS, E.FUZZ_SEED, crafted=True) == 0
    assert "%d cases identical, 0 skipped" % E.FUZZ_DRAWS in capsys.readouterr().out      # none of the fixed draws is an unsupported geometry
