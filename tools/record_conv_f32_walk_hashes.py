"""Record SHA-256 of every convolution output of a small f32 network on the shapes at which the scalar staging walk of k_conv_f32's two
unconditional tiles (<16, 2, 2, 4>, <16, 1, 2, 4>: buffer loads through two descriptors, k_yolo32.h) can go wrong:
tests/golden/conv_f32_walk_parent_hashes.json.

    python tools/record_conv_f32_walk_hashes.py <commit> [out.json]

Run it ONCE from a checkout of the commit whose results are the yardstick (the parent of the change) and name that commit;
tests/test_gpu_conv_f32_scalar_walk.py compares against the file, which is never regenerated from the code under test.  The network and the
cases are defined here and imported by the test (as tools/record_conv_f32_schedule_hashes.py does for its test, whose images(), digest() and key()
this module shares).

The network (walk_layers): the first layer and five stride-2 3 x 3 layers with 32 filters bring the map down to m = net / 32 (the detector API
admits net sizes that are multiples of 32); then, per layer: (filters, size / stride, stored input channels -> K steps, tile):
   6  160, 3 x 3 / 1, 32 -> 18 steps, on m: two filter tiles, the second partial (32 of 128)             <16, 2, 2, 4>
   7  96, 3 x 3 / 1, 160 -> 90 steps, on m: a partial filter tile, ten steps per tap                      <16, 2, 2, 4>
   8  64, 1 x 1, 96 -> 6 steps                                                                          <16, 1, 2, 4>
   9  64, 3 x 3 / 1, 64 -> 36 steps, linear, with the shortcut from 8                                     <16, 1, 2, 4>
  12  128, 1 x 1, 32 -> 2 steps (the fewest: the tile is at its end from the prologue on)                <16, 2, 2, 4>
  14  64, 1 x 1, 32 -> 2 steps, linear                                                                  <16, 1, 2, 4>
  16  128, 3 x 3 / 2, 32, from m to m / 2 (rounded up)                                                  <16, 2, 2, 4>
  18  64, 3 x 3 / 2, 32, from net / 16 to m                                                             <16, 1, 2, 4>
  20  128, 3 x 3 / 1, 32, on net / 16                                                                   <16, 2, 2, 4>
and the cases (net width, net height, batch):
  32 x 32, 1      m = 1 x 1, above it 2 x 2: the distance from a filter row's end to the next row is negative, the tile's anchor (tap (0, 0)
                  of its first pixel) lies in front of the tensor, eight of nine taps are padding
  96 x 96, 3      m = 3 x 3, above it 6 x 6: every tap-mask pattern of a 3 x 3 window; 27 and 108 pixels: one partial tile over three images
  640 x 480, 3    m = 20 x 15 at batch 3: 900 pixels = seven 128-pixel tiles and four pixels of an eighth; tiles 2 and 4 span two images
  352 x 224, 2    m = 11 x 7, an odd map under the stride-2 layer 16 (6 x 4 outputs); net / 16 = 22 x 14
A digest covers every image of the batch whole: the first and the last image's border tiles are in it."""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((32, 32, 1), (96, 96, 3), (640, 480, 3), (352, 224, 2))     # (network width, network height, batch)
SEED = 7
N_CONV = 15


def _schedule():
    spec = importlib.util.spec_from_file_location("sd_record_conv_f32_schedule_hashes", os.path.join(ROOT, "tools", "record_conv_f32_schedule_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_S = _schedule()
key, images, digest, conv_layers = _S.key, _S.images, _S.digest, _S.conv_layers


def walk_layers(pkg):
    """The layer list of the module's docstring as the detector takes it (yolo.LAYER_DTYPE)."""
    Y = pkg.yolo
    rows = []

    def conv(filters, size, stride, bn=1, leaky=1):
        rows.append(dict(type=Y.CONV, filters=filters, size=size, stride=stride, batch_normalize=bn, leaky=leaky))

    def route(a):
        rows.append(dict(type=Y.ROUTE, frm=a))

    def shortcut(a):
        rows.append(dict(type=Y.SHORTCUT, frm=a))

    conv(32, 3, 1)                                    # 0
    for _ in range(5):
        conv(32, 3, 2)                                # 1 - 5
    conv(160, 3, 1)                                   # 6
    conv(96, 3, 1)                                    # 7
    conv(64, 1, 1)                                    # 8
    conv(64, 3, 1, 1, 0); shortcut(-2)                # 9, 10
    route(5); conv(128, 1, 1)                         # 11, 12
    route(5); conv(64, 1, 1, 1, 0)                    # 13, 14
    route(5); conv(128, 3, 2)                         # 15, 16
    route(4); conv(64, 3, 2)                          # 17, 18
    route(4); conv(128, 3, 1)                         # 19, 20
    layers = np.zeros(len(rows), Y.LAYER_DTYPE)
    for L, r in zip(layers, rows):
        L["type"] = r["type"]
        if r["type"] == Y.CONV:
            for k in ("filters", "size", "stride", "batch_normalize", "leaky"):
                L[k] = r[k]
        else:
            L["from"][0] = r["frm"]; L["nfrom"] = 1
    return layers, np.asarray(pkg.yolo.v3_layers()[1], np.float32)


def forward_outputs(pkg, imgs, net_w, net_h):
    """{conv layer index: [len(imgs) arrays (h, w, c) f32]} of one f32 forward pass of walk_layers at net_w x net_h."""
    import torch
    layers, anchors = walk_layers(pkg)
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


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "conv_f32_walk_parent_hashes.json")
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
