"""Record SHA-256 of every convolution output of a small f32 network on the shapes at which k_conv_f32's K step can go wrong and the other
recorded hashes do not reach: tests/golden/conv_f32_schedule_parent_hashes.json.

    python tools/record_conv_f32_schedule_hashes.py <commit> [out.json]

Run it ONCE from a checkout of the commit whose results are the yardstick (the parent of a change to k_conv_f32's K loop) and name that commit;
tests/test_gpu_conv_f32_schedule.py compares against the file, which is never regenerated from the code under test.  The network and the cases
are defined here and imported by the test, so that both walk the same inputs (as tools/record_conv_f32_setup_hashes.py does for its test).

The network (schedule_layers) is a chain of five stride-2 3 x 3 layers with 32 filters behind the first layer -- the detector API admits net sizes
that are multiples of 32, so a 1 x 1, 2 x 2 or 3 x 3 map of 32 stored channels exists only 32 times down -- and, on the smallest map m (net / 32)
and the one above it (net / 16), one layer per property; per layer: (filters, size / stride, stored input channels -> K steps, tile):
   0  first layer, `pair` form: five K steps, a tap change every step                                   <8, 1, 1, 8>
   1 - 5   32, 3 x 3 / 2, 32 -> 18 steps; outputs net / 2 ... net / 32                                  <16, 1, 1, 4>
   6  128, 3 x 3 / 1, 32 -> 18 steps, on m                                                              <16, 2, 2, 4>
   8  64, 3 x 3 / 1, 32 -> 18 steps, on m                                                               <16, 1, 2, 4>
   9  64, 1 x 1, 64 -> 4 steps, linear, with the shortcut from 8                                        <16, 1, 2, 4>
  11  255, 1 x 1, 64 -> 4 steps, linear                                                                 <16, 2, 2, 4>
  13  255, 1 x 1, 32 -> 2 steps (the fewest: every step of the loop requests the zero page), linear, with the shortcut from 11
  16  64, 1 x 1, 32 -> 2 steps, leaky
  18  128, 3 x 3 / 2, 32, from net / 16 to m
  20  64, 3 x 3 / 1, 32, on net / 16
  22  128, 3 x 3 / 1, 128 -> 72 steps, on m: the steady state with all its tap changes
  23  128, 1 x 1, 128 -> 8 steps, leaky, with the shortcut from 22
and the cases (net width, net height, batch):
  32 x 32, 1     m = 1 x 1, above it 2 x 2: eight of nine taps are padding on m; the stride-2 layers read 2 x 2 and 4 x 4 maps
  96 x 96, 3     m = 3 x 3, above it 6 x 6: every tap-mask pattern of a 3 x 3 window; 27 and 108 pixels in 128- and 256-pixel tiles, i.e. one
                 partial tile whose later chunks lie beyond the last pixel
  640 x 480, 2   m = 20 x 15 at batch 2: 600 pixels = four full 128-pixel tiles and a partial fifth, layer 22's full walk; the first layer on
                 1200 pixel tiles"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((32, 32, 1), (96, 96, 3), (640, 480, 2))     # (network width, network height, batch)
SEED = 5


def key(nw, nh, batch):
    return "%dx%d n=%d" % (nw, nh, batch)


def schedule_layers(pkg):
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
    conv(128, 3, 1)                                   # 6
    route(5); conv(64, 3, 1)                          # 7, 8
    conv(64, 1, 1, 1, 0); shortcut(-2)                # 9, 10
    conv(255, 1, 1, 0, 0)                             # 11
    route(5); conv(255, 1, 1, 0, 0); shortcut(11)     # 12, 13, 14
    route(5); conv(64, 1, 1)                          # 15, 16
    route(4); conv(128, 3, 2)                         # 17, 18
    route(4); conv(64, 3, 1)                          # 19, 20
    route(6); conv(128, 3, 1)                         # 21, 22
    conv(128, 1, 1); shortcut(-2)                     # 23, 24
    layers = np.zeros(len(rows), Y.LAYER_DTYPE)
    for L, r in zip(layers, rows):
        L["type"] = r["type"]
        if r["type"] == Y.CONV:
            for k in ("filters", "size", "stride", "batch_normalize", "leaky"):
                L[k] = r[k]
        else:
            L["from"][0] = r["frm"]; L["nfrom"] = 1
    return layers, np.asarray(pkg.yolo.v3_layers()[1], np.float32)


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
    """{conv layer index: [len(imgs) arrays (h, w, c) f32]} of one f32 forward pass of schedule_layers at net_w x net_h."""
    import torch
    layers, anchors = schedule_layers(pkg)
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
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "conv_f32_schedule_parent_hashes.json")
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
