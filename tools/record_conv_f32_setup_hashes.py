"""Record SHA-256 of every convolution output of the f32 detector on inputs that stress k_conv_f32's set-up and tap change:
tests/golden/conv_f32_setup_parent_hashes.json.

    python tools/record_conv_f32_setup_hashes.py <commit> [out.json]

Run it ONCE from a checkout of the commit whose results are the yardstick (the parent of a change to k_conv_f32's set-up) and name that
commit; tests/test_gpu_conv_f32_setup.py compares against the file, which is never regenerated from the code under test.  The cases are
defined here and imported by the test, so that both walk the same inputs (as tools/record_conv_f32_hashes.py does for its test):
  64x32 at batch 5   maps 16x8 .. 2x1: on the 2x1 map both outer rows and one outer column of every 3x3 window are padding at once, the
                     stride-2 layer in front of it reads a 4x2 map, and five images make the pixel tiles straddle images differently
                     from the batch of three of the other test
  32x32 at batch 1   the deepest map is 1x1: eight of nine taps are padding for every pixel (and W - ksize + 1 is negative)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((64, 32, 5), (32, 32, 1))     # (network width, network height, batch)
SEED = 3


def key(nw, nh, batch):
    return "%dx%d n=%d" % (nw, nh, batch)


def images(synth, batch):
    """`batch` different synthetic images: frames of one synthetic sequence, every second one flipped (rows, then columns)."""
    cfg = synth.KITTI03_RGBD
    imgs = [np.ascontiguousarray(synth.rgbd_frame(6, k, cfg)[0][:, :, ::-1]) for k in range(batch)]
    for k in range(1, batch, 2):
        imgs[k] = np.ascontiguousarray(imgs[k][::-1] if k % 4 == 1 else imgs[k][:, ::-1])
    return imgs


def conv_layers(pkg, layers):
    return [i for i, l in enumerate(layers) if int(l["type"]) == pkg.yolo.CONV]


def forward_outputs(pkg, imgs, net_w, net_h):
    """{conv layer index: [len(imgs) arrays (h, w, c) f32]} of one f32 forward pass of the full v3 network at net_w x net_h."""
    import torch
    layers, anchors = pkg.yolo.v3_layers()
    payload, _ = pkg.yolo.synth_weights(layers, seed=SEED)
    H, W = imgs[0].shape[:2]
    n = len(imgs)
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    d = pkg.yolo.Detector(layers, anchors, net_w, net_h, max_batch=n, precision="f32")
    try:
        d.load_weights(payload)
        d.forward_device(dev.data_ptr(), W, H, W * 3, W * H * 3, n, 0.3)
        torch.cuda.synchronize()
        return {li: [d.layer_output(li, image=k) for k in range(n)] for li in conv_layers(pkg, layers)}
    finally:
        d.close()


def digest(per_image):
    h = hashlib.sha256()
    for a in per_image:
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "conv_f32_setup_parent_hashes.json")
    rec = {"commit": commit, "precision": "f32", "weights_seed": SEED, "cases": {}}
    for (nw, nh, batch) in CASES:
        outs = forward_outputs(pkg, images(pkg.synth, batch), nw, nh)
        rec["cases"][key(nw, nh, batch)] = {str(li): digest(v) for li, v in sorted(outs.items())}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("%s: %s" % (out, ", ".join("%s: %d layers" % (k, len(v)) for k, v in rec["cases"].items())))


if __name__ == "__main__":
    main()
