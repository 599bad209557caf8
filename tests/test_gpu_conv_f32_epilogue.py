"""k_conv_f32's prologue / epilogue on every convolution of the full YOLOv3 list, at two small network sizes whose maps leave partial pixel
tiles on every tile class (40x24 maps x 3 images = 22.5 tiles of 128 pixels; 3x2 maps x 3 = 18 pixels in one tile), with the 255-filter
heads, layers with and without a shortcut, leaky on and off, the in-place route outputs (outStride != cout), 1x1 layers of 2, 4, 8 and more
K steps and 3x3 layers of stride 1 and 2.  Two checks per convolution output, all 75 of them:
  1. within the suite's 2e-5 relative L2 of the torch-fp32 forward (oracle/yolo_oracle.py);
  2. bit for bit what the parent commit computed: SHA-256 against tests/golden/conv_f32_parent_hashes.json, recorded once on the GPU from
     a checkout of the commit the file names (tools/record_conv_f32_hashes.py) -- the epilogue's arithmetic is x = acc + bias, leaky, + shortcut
     in that order, and a change of tile geometry, staging order or store form must not move a bit."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _recorder():
    spec = importlib.util.spec_from_file_location("sd_record_conv_f32_hashes", os.path.join(ROOT, "tools", "record_conv_f32_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_f32_parent_hashes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rec():
    return _recorder()


@pytest.fixture(scope="module", params=["160x96", "96x64"])
def forward(request, gpu, pkg, synth, rec):
    """One forward pass per network size, shared by both checks: (size key, net_w, net_h, images, {layer: [outputs per image]})."""
    nw, nh = (int(v) for v in request.param.split("x"))
    assert (nw, nh) in rec.NET_SIZES
    imgs = rec.images(synth)
    return request.param, nw, nh, imgs, rec.forward_outputs(pkg, imgs, nw, nh)


def test_every_convolution_within_the_f32_bar_of_the_torch_forward(forward, pkg, orc):
    import __graft_entry__ as graft
    yo = graft.load_yolo_oracle()
    key, nw, nh, imgs, outs = forward
    layers, _ = pkg.yolo.v3_layers()
    _, per = pkg.yolo.synth_weights(layers, seed=3)
    assert len(outs) == 75
    worst = (0.0, None)
    for k in range(len(imgs)):
        ref = yo.torch_forward(layers, per, yo.blob_from_image(imgs[k], nw, nh, orc.resize_linear))
        for li, per_image in outs.items():
            got = per_image[k].transpose(2, 0, 1)
            # a [shortcut] is fused into the epilogue of the convolution before it (every one of yolov3.cfg is): that convolution's output
            # tensor holds the shortcut layer's values, so the shortcut reads and the add are compared too
            fused = li + 1 < len(layers) and int(layers[li + 1]["type"]) == pkg.yolo.SHORTCUT
            exp = ref[li + 1 if fused else li][0].numpy()
            assert got.shape == exp.shape, (key, li)
            e = _rel(got, exp)
            worst = max(worst, (e, (k, li)))
            assert e < 2e-5, "%s, image %d, layer %d: relative L2 error %.3g" % (key, k, li, e)
    print("%s: worst relative L2 error %.3g at (image, layer) %s" % (key, worst[0], worst[1]))


def test_every_convolution_bit_identical_to_the_parent_commit(forward, golden, rec):
    key, nw, nh, imgs, outs = forward
    assert (golden["precision"], golden["batch"], golden["weights_seed"]) == ("f32", rec.BATCH, rec.SEED)
    want = golden["sizes"][key]
    assert sorted(int(k) for k in want) == sorted(outs) and len(want) == 75
    moved = [li for li in sorted(outs) if rec.digest(outs[li]) != want[str(li)]]
    assert not moved, "%s: convolution outputs differ from commit %s at layers %s" % (key, golden["commit"][:12], moved)
