"""k_conv_f32's K step (every stage requested unconditionally, the tile's end folded into the tap change, staging placed among the MFMAs) on the
shapes at which it can go wrong and the other recorded hashes do not reach.

A small f32 network (tools/record_conv_f32_schedule_hashes.py: schedule_layers, the table of its layers is in that module's docstring) at three
sizes.  Per convolution output the two checks of tests/test_gpu_conv_f32_setup.py: within the suite's 2e-5 relative L2 of the torch-fp32 forward,
and bit for bit what the parent commit computed (SHA-256 against tests/golden/conv_f32_schedule_parent_hashes.json, recorded once on the GPU
from a build of the commit the file names, never regenerated from the code under test).  What the cases hold:
  fewest K steps        1 x 1 with 32 and 64 stored input channels (2 and 4 steps: every step of the loop requests the zero page), 255 and 64
                        filters, with and without a shortcut, leaky and linear (layers 9, 11, 13, 16);
  tiny maps             3 x 3 with 32 channels, stride 1 on 1 x 1, 2 x 2, 3 x 3 and 6 x 6 maps, stride 2 onto 1 x 1, 2 x 2 and 3 x 3 maps: every tap-mask
                        pattern, the zero page at every tap (layers 4, 5, 6, 8, 18, 20 at 32 x 32 and 96 x 96);
  partial tiles         96 x 96 at batch 3: 27 and 108 pixels, chunks beyond the last pixel; 640 x 480 at batch 2: 600 pixels, four full tiles and
                        a partial one;
  first layer           `pair` form, five steps, a tap change every step, at the smallest size the detector admits (32 x 32; the API takes net
                        sizes that are multiples of 32) and at 640 x 480;
  full walk             128 filters, 3 x 3, 128 channels on the 20 x 15 map at batch 2: 72 steps with all tap changes (layer 22), and the 1 x 1
                        128 -> 128 layer with a shortcut behind it (8 steps, layer 23)."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
N_CONV = 16


def _recorder():
    spec = importlib.util.spec_from_file_location("sd_record_conv_f32_schedule_hashes", os.path.join(ROOT, "tools", "record_conv_f32_schedule_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_f32_schedule_parent_hashes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rec():
    return _recorder()


@pytest.fixture(scope="module", params=["32x32 n=1", "96x96 n=3", "640x480 n=2"])
def forward(request, gpu, pkg, synth, rec):
    """One forward pass per case, shared by both checks: (case key, net_w, net_h, images, {layer: [outputs per image]})."""
    case = {rec.key(*c): c for c in rec.CASES}[request.param]
    nw, nh, batch = case
    imgs = rec.images(synth, batch)
    return request.param, nw, nh, imgs, rec.forward_outputs(pkg, imgs, nw, nh)


def test_every_convolution_within_the_f32_bar_of_the_torch_forward(forward, pkg, orc, rec):
    import __graft_entry__ as graft
    yo = graft.load_yolo_oracle()
    key, nw, nh, imgs, outs = forward
    layers, _ = rec.schedule_layers(pkg)
    _, per = pkg.yolo.synth_weights(layers, seed=rec.SEED)
    assert len(outs) == N_CONV
    worst = (0.0, None)
    for k in range(len(imgs)):
        ref = yo.torch_forward(layers, per, yo.blob_from_image(imgs[k], nw, nh, orc.resize_linear))
        for li, per_image in outs.items():
            got = per_image[k].transpose(2, 0, 1)
            # a [shortcut] is fused into the epilogue of the convolution before it: that convolution's tensor holds the shortcut layer's values
            fused = li + 1 < len(layers) and int(layers[li + 1]["type"]) == pkg.yolo.SHORTCUT
            exp = ref[li + 1 if fused else li][0].numpy()
            assert got.shape == exp.shape, (key, li)
            assert np.abs(exp).max() > 0, "%s, layer %d: the reference is all zeros" % (key, li)
            e = _rel(got, exp)
            worst = max(worst, (e, (k, li)))
            assert e < 2e-5, "%s, image %d, layer %d: relative L2 error %.3g" % (key, k, li, e)
    print("%s: worst relative L2 error %.3g at (image, layer) %s" % (key, worst[0], worst[1]))


def test_every_convolution_bit_identical_to_the_parent_commit(forward, golden, rec):
    key, nw, nh, imgs, outs = forward
    assert (golden["precision"], golden["weights_seed"]) == ("f32", rec.SEED)
    want = golden["cases"][key]
    assert sorted(int(k) for k in want) == sorted(outs) and len(want) == N_CONV
    moved = [li for li in sorted(outs) if rec.digest(outs[li]) != want[str(li)]]
    assert not moved, "%s: convolution outputs differ from commit %s at layers %s" % (key, golden["commit"][:12], moved)
