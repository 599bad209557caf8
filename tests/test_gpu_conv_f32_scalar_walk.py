"""k_conv_f32's scalar staging walk (buffer loads through two descriptors per workgroup, a 32-bit offset per lane, the K walk in scalar
registers; the two unconditional tiles <16, 2, 2, 4> and <16, 1, 2, 4>) on the smallest shapes at which it can go wrong.

A small f32 network (tools/record_conv_f32_walk_hashes.py: walk_layers; the table of its layers and what each case holds are in that module's
docstring) at four sizes.  Every convolution output is bit for bit what the parent commit computed: SHA-256 over all images of the batch (the first
and the last image's border tiles included) against tests/golden/conv_f32_walk_parent_hashes.json, recorded once on the GPU from a build of the
commit the file names, never regenerated from the code under test.  What the cases hold:
  tiny maps             3 x 3 filters on 1 x 1, 2 x 2, 3 x 3 and 6 x 6 maps: the row distance of the tap walk is negative, the tile's anchor lies in front
                        of the tensor, most taps are padding and answer zeros through the descriptor's range check;
  tiles across images   20 x 15 at batch 3: 900 pixels, tiles that span two images, a last tile of four pixels;
  odd map, stride 2     11 x 7 -> 6 x 4 (layer 16 at 352 x 224);
  K depth               32 stored input channels (two-step 1 x 1 tiles: at their end from the prologue on, layers 12 and 14), 160 (ten steps per
                        tap, layer 7);
  partial filter tiles  160 and 96 filters (layers 6 and 7);
  the 64-filter tile    1 x 1, 3 x 3 with a fused shortcut, stride 2 (layers 8, 9, 14, 18).
The guard for anchors beyond 4 GiB is the large-tensor case of tests/test_gpu_conv_f32_setup.py."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _recorder():
    spec = importlib.util.spec_from_file_location("sd_record_conv_f32_walk_hashes", os.path.join(ROOT, "tools", "record_conv_f32_walk_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_f32_walk_parent_hashes.json")) as f:
        g = json.load(f)
    assert len(g["commit"]) == 40
    return g


@pytest.fixture(scope="module")
def rec():
    return _recorder()


@pytest.mark.parametrize("case", ["32x32 n=1", "96x96 n=3", "640x480 n=3", "352x224 n=2"])
def test_every_convolution_bit_identical_to_the_parent_commit(case, gpu, pkg, synth, rec, golden):
    nw, nh, batch = {rec.key(*c): c for c in rec.CASES}[case]
    assert (golden["precision"], golden["weights_seed"]) == ("f32", rec.SEED)
    outs = rec.forward_outputs(pkg, rec.images(synth, batch), nw, nh)
    want = golden["cases"][case]
    assert sorted(int(k) for k in want) == sorted(outs) and len(want) == rec.N_CONV
    assert all(v[0].size > 0 and abs(v[-1]).max() > 0 for v in outs.values()), "an output is empty or all zeros"
    moved = [li for li in sorted(outs) if rec.digest(outs[li]) != want[str(li)]]
    assert not moved, "%s: convolution outputs differ from commit %s at layers %s" % (case, golden["commit"][:12], moved)
