"""Record SHA-256 of every convolution output of the f32 detector on the GPU: tests/golden/conv_f32_parent_hashes.json.

    python tools/record_conv_f32_hashes.py <commit> [out.json]

Run it ONCE from a checkout of the commit whose results are the yardstick (the parent of a change to k_conv_f32) and name that commit; the
file is then compared against by tests/test_gpu_conv_f32_epilogue.py and never regenerated from the code under test.  The cases (network
sizes, batch, weights, images) are defined here and imported by the test, so that both walk the same inputs."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_SIZES = ((160, 96), (96, 64))      # feature maps 40x24 .. 5x3 and 24x16 .. 3x2: partial pixel tiles on every tile class
BATCH = 3
SEED = 3


def images(synth):
    """Three different synthetic images, as tests/test_gpu_yolo.py::test_f32_modes_odd_feature_maps_and_batch makes them."""
    cfg = synth.KITTI03_RGBD
    imgs = [np.ascontiguousarray(synth.rgbd_frame(6, k, cfg)[0][:, :, ::-1]) for k in range(BATCH)]
    imgs[1] = np.ascontiguousarray(imgs[1][::-1]); imgs[2] = np.ascontiguousarray(imgs[2][:, ::-1])
    return imgs


def conv_layers(pkg, layers):
    return [i for i, l in enumerate(layers) if int(l["type"]) == pkg.yolo.CONV]


def forward_outputs(pkg, imgs, net_w, net_h):
    """{conv layer index: [BATCH arrays (h, w, c) f32]} of one f32 forward pass of the full v3 network at net_w x net_h."""
    import torch
    layers, anchors = pkg.yolo.v3_layers()
    payload, _ = pkg.yolo.synth_weights(layers, seed=SEED)
    H, W = imgs[0].shape[:2]
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    d = pkg.yolo.Detector(layers, anchors, net_w, net_h, max_batch=BATCH, precision="f32")
    try:
        d.load_weights(payload)
        d.forward_device(dev.data_ptr(), W, H, W * 3, W * H * 3, BATCH, 0.3)
        torch.cuda.synchronize()
        return {li: [d.layer_output(li, image=k) for k in range(BATCH)] for li in conv_layers(pkg, layers)}
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
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "conv_f32_parent_hashes.json")
    imgs = images(pkg.synth)
    rec = {"commit": commit, "precision": "f32", "batch": BATCH, "weights_seed": SEED, "sizes": {}}
    for (nw, nh) in NET_SIZES:
        outs = forward_outputs(pkg, imgs, nw, nh)
        rec["sizes"]["%dx%d" % (nw, nh)] = {str(li): digest(v) for li, v in sorted(outs.items())}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("%s: %s" % (out, ", ".join("%s: %d layers" % (k, len(v)) for k, v in rec["sizes"].items())))


if __name__ == "__main__":
    main()
