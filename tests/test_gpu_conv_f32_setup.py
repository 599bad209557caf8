"""k_conv_f32's set-up and tap change (multiply-high pixel split, incremental tap pointers, tap masks) on inputs that stress them.

Every convolution of the full YOLOv3 list, the same two checks per output as tests/test_gpu_conv_f32_epilogue.py -- within the suite's 2e-5
relative L2 of the torch-fp32 forward, and bit for bit what the parent commit computed (SHA-256 against
tests/golden/conv_f32_setup_parent_hashes.json, recorded once on the GPU from a checkout of the commit the file names by
tools/record_conv_f32_setup_hashes.py, never regenerated from the code under test) -- on
  64x32 at batch 5   maps 16x8 .. 2x1: on the 2x1 map both outer rows of a 3x3 window and one of its outer columns are padding at once, a
                     stride-2 layer reads a 4x2 map, and five images make the pixel tiles straddle images differently from a batch of three;
  32x32 at batch 1   the deepest map is 1x1: eight of nine taps are padding for every pixel, and the distance from a filter row's last tap to
                     the next row's first is negative.
And one addressing test at the benchmark's own scale, which no small shape can replace: at batch 256 the outputs of the first layers exceed
2^31 elements, so the first and the last image of one 640x480 pass must equal, bit for bit, a batch-1 pass on the same image."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _recorder():
    spec = importlib.util.spec_from_file_location("sd_record_conv_f32_setup_hashes", os.path.join(ROOT, "tools", "record_conv_f32_setup_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_f32_setup_parent_hashes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rec():
    return _recorder()


@pytest.fixture(scope="module", params=["64x32 n=5", "32x32 n=1"])
def forward(request, gpu, pkg, synth, rec):
    """One forward pass per case, shared by both checks: (case key, net_w, net_h, images, {layer: [outputs per image]})."""
    case = {rec.key(*c): c for c in rec.CASES}[request.param]
    nw, nh, batch = case
    imgs = rec.images(synth, batch)
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
            # a [shortcut] is fused into the epilogue of the convolution before it: that convolution's tensor holds the shortcut layer's values
            fused = li + 1 < len(layers) and int(layers[li + 1]["type"]) == pkg.yolo.SHORTCUT
            exp = ref[li + 1 if fused else li][0].numpy()
            assert got.shape == exp.shape, (key, li)
            e = _rel(got, exp)
            worst = max(worst, (e, (k, li)))
            assert e < 2e-5, "%s, image %d, layer %d: relative L2 error %.3g" % (key, k, li, e)
    print("%s: worst relative L2 error %.3g at (image, layer) %s" % (key, worst[0], worst[1]))


def test_every_convolution_bit_identical_to_the_parent_commit(forward, golden, rec):
    key, nw, nh, imgs, outs = forward
    assert (golden["precision"], golden["weights_seed"]) == ("f32", rec.SEED)
    want = golden["cases"][key]
    assert sorted(int(k) for k in want) == sorted(outs) and len(want) == 75
    moved = [li for li in sorted(outs) if rec.digest(outs[li]) != want[str(li)]]
    assert not moved, "%s: convolution outputs differ from commit %s at layers %s" % (key, golden["commit"][:12], moved)


def test_batch_256_addresses_beyond_2_31_elements(gpu, pkg, synth):
    """640x480, f32: layer 0 writes 256 x 640 x 480 x 32 = 2.5e9 floats and layer 1 reads them.  Images 0 and 255 of a batch-256 pass (the same
    picture in every slot) must equal the batch-1 pass bit for bit at layers 0, 1, 3 and 5."""
    import torch
    layers, anchors = pkg.yolo.v3_layers()
    payload, _ = pkg.yolo.synth_weights(layers, seed=3)
    cfg = synth.KITTI03_RGBD
    img = np.ascontiguousarray(synth.rgbd_frame(6, 0, cfg)[0][:, :, ::-1])
    H, W = img.shape[:2]
    probe = (0, 1, 3, 5)

    def run(batch, images):
        dev = torch.from_numpy(img).cuda().unsqueeze(0).expand(batch, -1, -1, -1).contiguous()
        d = pkg.yolo.Detector(layers, anchors, 640, 480, max_batch=batch, precision="f32")
        try:
            d.load_weights(payload)
            d.forward_device(dev.data_ptr(), W, H, W * 3, W * H * 3, batch, 0.3)
            torch.cuda.synchronize()
            return {(li, k): d.layer_output(li, image=k) for li in probe for k in images}
        finally:
            d.close()

    one = run(1, (0,))
    big = run(256, (0, 255))
    for li in probe:
        assert np.abs(one[(li, 0)]).max() > 0, "layer %d: the reference pass is all zeros" % li
        for k in (0, 255):
            assert big[(li, k)].tobytes() == one[(li, 0)].tobytes(), "layer %d: image %d of the batch of 256 differs from the batch-1 pass" % (li, k)
