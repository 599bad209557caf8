"""The three Levenberg-Marquardt kernels (k_pose_optimize, k_local_ba, k_sim3_optimize), the ComputeSim3 refine chain and the
relocalisation cascade answer bit for bit what the parent commit of csrc/sd_g2o_math.h answered, on the crafted cases the project already
has (tools/record_lm_hashes.py: the groups, and what each digest covers, are in that module's docstring).  One SHA-256 per case over the
bytes of every output array, against tests/golden/lm_parent_hashes.json: recorded once on the GPU from a build of the commit the file
names, never regenerated from the code under test.  No tolerance: the solvers' arithmetic moved into one header and must not have changed."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _recorder():
    spec = importlib.util.spec_from_file_location("sd_record_lm_hashes", os.path.join(ROOT, "tools", "record_lm_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _recorder()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "lm_parent_hashes.json")) as f:
        g = json.load(f)
    assert len(g["commit"]) == 40 and sorted(g["cases"]) == sorted(rec.GROUPS)
    return g


@pytest.fixture(scope="module")
def ws(gpu, fe, synth):
    w = rec.workspace(fe, synth)
    yield w
    w.close()


def _compare(golden, group, got):
    want = golden["cases"][group]
    assert sorted(got) == sorted(want) and len(want) > 0, "%s: the case list is not the recorded one" % group
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, "%s: %d of %d cases differ from commit %s: %s" % (group, len(moved), len(want), golden["commit"][:12], moved[:12])


@pytest.mark.parametrize("group", [g.__name__ for g in rec.PLAIN])
def test_plain_entries_bit_identical_to_the_parent_commit(group, gpu, fe, synth, golden):
    _compare(golden, group, getattr(rec, group)(fe, synth))


@pytest.mark.parametrize("group", [g.__name__ for g in rec.ON_WORKSPACE])
def test_batch_entries_bit_identical_to_the_parent_commit(group, ws, fe, synth, golden):
    _compare(golden, group, getattr(rec, group)(fe, synth, ws))
