"""Crafted detector networks, their float64 reference and the derived elementwise error bound (tests/test_yolo_cases.py on the CPU,
tests/test_gpu_yolo_cases.py on the GPU).  No GPU code in here.

Every GPU test of the detector used to build its network from the stock yolov3 layer list, so most of what csrc/sd_yolo_plan.h can choose
never ran, and every check was a relative L2 norm over a whole tensor measured through the whole network.  The lists below are a few layers
deep and small; between them every kernel instantiation of SD_YOLO_KERNELS that can be reached is planned (tests/test_yolo_cases.py is the
arbiter), and every convolution is compared ELEMENT BY ELEMENT with a float64 evaluation of that one layer on the tensor the GPU itself fed it.

The reference of a layer (Case.reference_layer)
    uses the weights as the mode stores them -- batch norm folded in float32 exactly as sd_yolo_load_darknet_weights folds it,
    w * (gamma / sqrtf(var + 1e-6f)) and beta - mean * sc, then rounded to f16 in the f16 mode; the f32-class modes keep the f32 values (the
    three bf16 limbs of the f32x3 mode sum to the f32 value exactly) -- and adds bias, leaky ReLU (slope float32(0.1)) and the fused residual in
    float64.  A convolution followed by a fused [shortcut] holds the shortcut's values.  Mode "f64" folds in float64 and uses slope 0.1: the
    restatement of oracle/yolo_oracle.torch_forward(dtype=float64) that ties this module to the oracle the rest of the suite trusts.

The bound (Case.bound_layer), derived, not tuned.  u = 2^-24 (f32 unit round-off); A = conv(|x|, |w|) + |bias| + |residual|, the same
expression on absolute values; K = taps x real input channels.
    direct f32     a dot product of K terms summed in any order errs by at most K u A to first order (one rounding per product, one per sum);
                   the epilogue's bias add, slope multiply and residual add are three more roundings of values <= A.  K >= 27, so
                   K + 3 <= 2 K covers the unknown association inside the MFMA and the epilogue:          |got - ref| <= 2 K u A.
    f32x3          the same sum of limb products (each exact in f32) plus the dropped products mid*lo, lo*mid, lo*lo <= (2^-23 + 2^-32) |a b|:
                                                                                                           2 K u A + 2^-22.99 A  (written 2^-23 (1 + 2^-9) A).
    f16            operands are the stored f16 values, products exact, accumulators f32: the same accumulation term e = 2 K u A; then the
                   kernels round leaky(acc + bias) to f16, add the f16 residual in f32 and round again:
                   max(2^-11 |pre|, 2^-24) (fused shortcut only) + max(2^-11 |ref|, 2^-24) + e (1 + 2^-10) + 2^-23 |bias|
                   (2^-24: one f16 subnormal; 2^-23 |bias|: a bias folded with a fused multiply-add differs by one f32 ulp).  A layer whose weights
                   are not f16-exact needs nothing more: the reference already uses the rounded weights.
    Winograd       the f32w mode computes Y = A^T [ sum_c (G g G^T) . (B^T d B) ] A.  Its error is bounded by the same expression on absolute
                   values, A_w = |A^T| ( sum_c (|G| |g| |G^T|) . (|B^T| |d| |B|) ) |A| + |bias| + |residual|, times the number of roundings on
                   the longest path through it: 4 for U = G g G^T (two levels of two additions; the halvings are exact), 2 for V = B^T d B (one
                   addition per level), cin for the products and their sum over the channels of one position, 9 for the fold of the (at most)
                   nine positions into an output, 3 for the epilogue: n = cin + 18 in the place of K:      2 (cin + 18) u A_w.
                   (A_w >= A: the transforms' cancellations are what Winograd pays for its 2.25 x fewer multiplies.)
"""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV, SHORTCUT, ROUTE, UPSAMPLE, YOLO = 0, 1, 2, 3, 4
MODES = ("f16", "f32", "f32w", "f32x3")
PRECS = {"f16": 0, "f32": 1, "f32w": 2, "f32x3": 3}
SD_ERR_INVALID, SD_ERR_UNSUPPORTED = -1, -5
CLS_WINO = 3                        # SdYoloClass
U32 = 2.0 ** -24                    # f32 unit round-off
ANCHORS = np.array([10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326], np.float32)
# the layer record of the C ABI (slam-dynamic_amd/yolo.py LAYER_DTYPE; the GPU test asserts they are the same)
LAYER_DTYPE = np.dtype([("type", "<i4"), ("filters", "<i4"), ("size", "<i4"), ("stride", "<i4"), ("batch_normalize", "<i4"),
                        ("leaky", "<i4"), ("from", "<i4", (2,)), ("nfrom", "<i4"), ("mask", "<i4", (3,))])


def conv(filters, size=3, stride=1, bn=1, leaky=1):
    return (CONV, filters, size, stride, bn, leaky, (0, 0), 0, (0, 0, 0))


def head():
    return conv(255, 1, 1, bn=0, leaky=0)


def shortcut(frm):
    return (SHORTCUT, 0, 0, 0, 0, 0, (frm, 0), 1, (0, 0, 0))


def route(a, b=None):
    return (ROUTE, 0, 0, 0, 0, 0, (a, 0 if b is None else b), 1 if b is None else 2, (0, 0, 0))


def upsample():
    return (UPSAMPLE, 0, 0, 2, 0, 0, (0, 0), 0, (0, 0, 0))


def yolo(m0, m1, m2):
    return (YOLO, 0, 0, 0, 0, 0, (0, 0), 0, (m0, m1, m2))


def layer_array(ls):
    a = np.zeros(len(ls), LAYER_DTYPE)
    for i, l in enumerate(ls):
        a[i] = l
    return a


# ------------------------------------------------------------------------------------------------------------------------------------
# The lists.  What each is for stands beside its layers; which kernel a layer really gets is asserted by tests/test_yolo_cases.py.
# ------------------------------------------------------------------------------------------------------------------------------------
_PARTIAL = [                        # 96 x 64, batch 3: partial filter tiles (96, 160), input channels 32 / 96 / 160, the in-place route, two heads
    conv(32), conv(64, 3, 2),       # 0, 1 -> 48 x 32
    conv(32),                       # 2: the 32-filter tile on nine taps
    conv(64), shortcut(-3),         # 3, 4: input channels 32 behind the first layer; fused shortcut from layer 1
    conv(96, 3, 2),                 # 5 -> 24 x 16: a partial 128-filter tile
    conv(96), shortcut(-2),         # 6, 7: input channels 96, partial tile in the flat kernels, residual = its own input
    conv(160, 3, 2),                # 8 -> 12 x 8
    conv(128),                      # 9: input channels 160: Winograd with ten K steps per position, k_conv3x3_flat with five chunks
    head(), yolo(6, 7, 8),          # 10, 11
    route(-3), conv(32, 1), upsample(), route(-1, 7),      # 12 - 15: 32 + 96 channels at 24 x 16, the skip tensor written in place (f32-class modes)
    conv(64), head(), yolo(3, 4, 5)]                       # 16 - 18
_ODD = [                            # 160 x 96, batch 5: maps 80 x 48 ... 5 x 3 and 3 x 2, tiles that straddle images
    conv(32), conv(64, 3, 2),       # 0, 1 -> 80 x 48
    conv(128),                      # 2: 80 wide
    conv(64, 1),                    # 3
    conv(128, 3, 2),                # 4 -> 40 x 24
    conv(64, 1), conv(128), shortcut(-3),                  # 5, 6, 7
    conv(224, 3, 2),                # 8 -> 20 x 12: a partial tile of 224
    conv(32, 1),                    # 9: the 32-filter tile on input channels 224
    conv(256),                      # 10: input channels 32 on the flat kernels (one 32-channel chunk)
    conv(160, 3, 2),                # 11 -> 10 x 6
    conv(128),                      # 12: input channels 160
    conv(96, 3, 2),                 # 13 -> 5 x 3
    conv(128, 3, 1, bn=0),          # 14: 5 x 3, odd both ways: the Winograd blocks of the last row and column hang over the edge; input channels 96
    conv(128, 3, 2),                # 15 -> 3 x 2: a stride-2 layer reads the odd map
    head(), yolo(6, 7, 8),          # 16, 17
    route(-4), conv(64, 1), upsample(), route(-1, 12),     # 18 - 21: layer 14 -> 64 channels -> 10 x 6, + layer 12 in place
    conv(96), head(), yolo(3, 4, 5)]                       # 22 - 24: input channels 192, partial tile
_WIDE = [                           # 128 x 32, batch 1: the 160-wide kernels below their maximum width
    conv(32),
    conv(128),                      # 1: width 128: k_conv3x3_b3<8, 2, 2> with 7 staged pieces, k_conv3x3_glds<160>
    conv(128), shortcut(-2),        # 2, 3: the same with input channels 128 (Winograd at width 128) and a residual
    conv(128, 3, 2),                # 4 -> 64 x 16
    head(), yolo(0, 1, 2)]
_B3F5 = [                           # 352 x 32, batch 1: the one width class (81 ... 95) no network of at most 160 pixels reaches: k_conv3x3_b3<5, 2, 2>
    conv(32), conv(64, 3, 2), conv(128, 3, 2),             # -> 176 x 16 -> 88 x 8
    conv(128),                      # 3: width 88
    head(), yolo(0, 1, 2)]
_TINY = [                           # 32 x 32, batch 1 and 96: the deepest map is 1 x 1; at batch 96 every tile spans many images
    conv(32),
    conv(160),                      # 1: input channels 32, partial tile; the 8-wave LDS-DMA kernel at batch 96
    conv(224, 1),                   # 2: 1 x 1 on input channels 160
    conv(64, 3, 2),                 # 3 -> 16 x 16: input channels 224: k_conv_mfma<32> at batch 1
    conv(128),                      # 4
    conv(96, 3, 2),                 # 5 -> 8 x 8
    conv(128, 3, 2),                # 6 -> 4 x 4: input channels 96
    conv(128), shortcut(-2),        # 7, 8: a 4 x 4 map
    conv(256, 3, 2),                # 9 -> 2 x 2
    conv(128, 3, 2),                # 10 -> 1 x 1
    conv(128),                      # 11: 3 x 3 on a 1 x 1 map: eight of nine taps are padding
    head(), yolo(6, 7, 8)]          # 12, 13: 3 rows per image: 86 images in one k_region_decode workgroup at batch 96
_DENSE_ROUTE = [                    # 64 x 64, batch 2: the skip tensor (layer 1) is read by a second route, so no route may own it: k_upsample_concat in every mode
    conv(32), conv(64, 3, 2), conv(64, 3, 2), conv(32, 1), upsample(), route(-1, 1),       # 0 - 5: 32 + 64 channels at 32 x 32
    head(), yolo(3, 4, 5),          # 6, 7
    route(1), head(), yolo(0, 1, 2)]                       # 8 - 10
_NO_HEAD = [conv(32), conv(32), conv(64, 3, 2, bn=0)]      # 32 x 32, batch 2: no [yolo] layer: zero rows, zero boxes; layer 1: 32 filters on input channels 32 (k_conv_mfma<32> with one K chunk per tap)


class Case:
    def __init__(self, name, ls, net_w, net_h, batches, seed, head_gain=3.0, obj_bias=-1.0):
        self.name, self.layers, self.net_w, self.net_h, self.batches, self.seed = name, layer_array(ls), net_w, net_h, tuple(batches), seed
        self.head_gain, self.obj_bias = head_gain, obj_bias          # chosen per list so that a few boxes per image pass the filters (test_crafted_heads_yield_boxes)
        self.anchors = ANCHORS
        self._w = None

    def __repr__(self):
        return "Case(%s)" % self.name

    # ---- structure
    @property
    def convs(self):
        return [i for i, l in enumerate(self.layers) if l["type"] == CONV]

    @property
    def heads(self):
        return [i for i, l in enumerate(self.layers) if l["type"] == YOLO]

    def resolve(self, i, f):
        return i + int(f) if f < 0 else int(f)

    def fused(self, i):
        """The [shortcut] fused into convolution i's epilogue (its index), or None."""
        return i + 1 if i + 1 < len(self.layers) and self.layers[i + 1]["type"] == SHORTCUT else None

    def residual_of(self, i):
        s = self.fused(i)
        return None if s is None else self.resolve(s, self.layers[s]["from"][0])

    def cin(self, i):
        return conv_inputs(self.layers)[i]

    def taps_k(self, i):
        return int(self.layers[i]["size"]) ** 2 * self.cin(i)

    def is_wino(self, i, mode):
        """sd_yolo_plan.h's rule for SD_YC_WINO (tests/test_yolo_cases.py checks it against the planner's class column)."""
        l = self.layers[i]
        return mode == "f32w" and i > 0 and l["size"] == 3 and l["stride"] == 1 and self.cin(i) >= 64 and l["filters"] % 128 == 0

    # ---- weights and frames
    def weights(self):
        if self._w is None:
            self._w = crafted_weights(self.layers, self.seed, self.head_gain, self.obj_bias)
        return self._w

    def frames(self, batch):
        """Integer-valued BGR frames of the network's own size (blobFromImage is then pixel * (1 / 255)), every image different -- noise of its own
        contrast and brightness per image, so that the images still differ where a deep map has averaged the noise away; the frames of a smaller
        batch are the first ones of a larger batch."""
        out = []
        for k in range(batch):
            rng = np.random.default_rng([self.seed, 77, k])
            a = rng.uniform(0.15, 1.0)
            b = rng.uniform(0, 255 * (1 - a))
            out.append(np.floor(rng.integers(0, 256, (self.net_h, self.net_w, 3)) * a + b).astype(np.uint8))
        return np.stack(out)

    def blobs(self, frames, mode):
        """(n, H, W, 3) float64: what the first convolution reads: RGB * float32(1 / 255) in f32, rounded to f16 in the f16 mode (k_blob_from_image)."""
        b = frames[..., ::-1].astype(np.float32) * np.float32(1 / 255.0)
        if mode == "f16":
            b = b.astype(np.float16)
        return b.astype(np.float64)

    def stored(self, i, mode):
        """(w [F, cin, k, k], bias [F]) of convolution i as float64 VALUES of what the mode stores (mode "f64": folded in float64)."""
        l, p = self.layers[i], self.weights()[1][i]
        if l["batch_normalize"]:
            if mode == "f64":
                sc = p["gamma"].astype(np.float64) / np.sqrt(p["var"].astype(np.float64) + 1e-6)
                w = p["w"].astype(np.float64) * sc[:, None, None, None]
                b = p["beta"].astype(np.float64) - p["mean"].astype(np.float64) * sc
            else:
                sc = p["gamma"] / np.sqrt(p["var"] + np.float32(1e-6))          # float32 throughout, as the loader
                w = p["w"] * sc[:, None, None, None]
                b = p["beta"] - p["mean"] * sc
                assert w.dtype == np.float32 and b.dtype == np.float32
        else:
            w, b = p["w"], p["bias"]
        if mode == "f16":
            w = w.astype(np.float16)
        return w.astype(np.float64), b.astype(np.float64)

    # ---- one layer
    def evaluate(self, i, x, mode, res=None):
        """LayerEval of convolution i on input x (n, H, W, cin) with the fused residual res (n, Ho, Wo, F) or None."""
        return LayerEval(self, i, np.asarray(x, np.float64), mode, None if res is None else np.asarray(res, np.float64))

    def reference_layer(self, i, x, mode, res=None):
        return self.evaluate(i, x, mode, res).out

    def bound_layer(self, i, x, mode, res=None):
        return self.evaluate(i, x, mode, res).bound()

    # ---- the whole list, layer by layer
    def forward_reference(self, frames, mode, storage=True, evals=None):
        """Chains reference_layer over the list -> per layer (n, H, W, C) float64 (None for [upsample]); a convolution with a fused shortcut and
        the shortcut hold the sum.  storage: round every convolution's output to the mode's activation type (what the next layer would read on
        the GPU); mode "f64" never rounds.  evals: a dict that receives every convolution's LayerEval."""
        outs = []
        x = self.blobs(frames, mode)
        for i, l in enumerate(self.layers):
            t = int(l["type"])
            if t == CONV:
                r = self.residual_of(i)
                ev = self.evaluate(i, x, mode, None if r is None else outs[r])
                if evals is not None:
                    evals[i] = ev
                x = ev.out
                if storage and mode != "f64":
                    x = x.astype(np.float16 if mode == "f16" else np.float32).astype(np.float64)
            elif t == SHORTCUT:
                x = outs[i - 1]
            elif t == ROUTE:
                src = [self.resolve(i, f) for f in l["from"][:int(l["nfrom"])]]
                if len(src) == 2:
                    x = np.concatenate([upsample2(outs[src[0] - 1]), outs[src[1]]], -1)
                else:
                    x = outs[src[0]]
            elif t == UPSAMPLE:
                outs.append(None)
                continue
            elif t == YOLO:
                x = outs[i - 1]
            outs.append(x)
        return outs


def upsample2(x):
    return x.repeat(2, axis=1).repeat(2, axis=2)


def conv_inputs(layers):
    """Input channel count of every convolution (3 for the first)."""
    c, out_c, cins = 3, [], {}
    for i, l in enumerate(layers):
        t = int(l["type"])
        if t == CONV:
            cins[i] = c
            c = int(l["filters"])
        elif t == ROUTE:
            c = sum(out_c[i + int(f) if f < 0 else int(f)] for f in l["from"][:int(l["nfrom"])])
        out_c.append(c)
    return cins


def crafted_weights(layers, seed, head_gain=3.0, obj_bias=-1.0):
    """Darknet payload (as slam_dynamic_amd.yolo.synth_weights lays it out) and the per-convolution arrays.  |w| is drawn from [0.5, 1] s with a
    random sign, so no product term of a dot product is negligible beside the others and a dropped tap stays visible; s keeps the activations
    O(1) through the list.  The weights of a convolution without batch norm are f16 values (the f16 mode stores them without rounding)."""
    rng = np.random.default_rng([seed, 5])
    cins = conv_inputs(layers)
    parts, per = [], {}
    for i, l in enumerate(layers):
        if l["type"] != CONV:
            continue
        F, k, cin = int(l["filters"]), int(l["size"]), cins[i]
        is_head = F == 255 and not l["leaky"]
        s = (head_gain if is_head else 1.85) / np.sqrt(cin * k * k)
        w = (rng.uniform(0.5, 1.0, (F, cin, k, k)) * rng.choice([-1.0, 1.0], (F, cin, k, k)) * s).astype(np.float32)
        if l["batch_normalize"]:
            beta = rng.normal(0, 0.05, F).astype(np.float32)
            gamma = rng.uniform(0.9, 1.1, F).astype(np.float32)
            mean = rng.normal(0, 0.05, F).astype(np.float32)
            var = rng.uniform(0.8, 1.2, F).astype(np.float32)
            parts += [beta, gamma, mean, var, w.reshape(-1)]
            per[i] = dict(w=w, beta=beta, gamma=gamma, mean=mean, var=var)
        else:
            w = w.astype(np.float16).astype(np.float32)
            bias = rng.normal(0, 0.2, F).astype(np.float32)
            if is_head:
                bias[4::85] += obj_bias     # objectness prior
                for c in (0, 2, 5):         # person / car / bus favoured: the class filter keeps some boxes
                    bias[5 + c::85] += 3.0
            parts += [bias, w.reshape(-1)]
            per[i] = dict(w=w, bias=bias)
    return np.concatenate(parts).astype(np.float32), per


# Winograd F(2 x 2, 3 x 3) as csrc/k_yolo32w.h computes it
_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def _conv_nhwc(x, w, stride):
    """sum over the taps of (pixels x cin) @ (cin x F): (n, H, W, cin), (F, cin, k, k) -> (n, Ho, Wo, F), padding k // 2, float64."""
    n, H, W, _ = x.shape
    F, _, k, _ = w.shape
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0))) if pad else x
    z = np.zeros((n, Ho, Wo, F), np.float64)
    for kh in range(k):
        for kw in range(k):
            tap = np.ascontiguousarray(xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :]).reshape(-1, x.shape[-1])
            z += (tap @ np.ascontiguousarray(w[:, :, kh, kw].T)).reshape(z.shape)
    return z


class LayerEval:
    """One convolution in float64: z = conv(x, w) + bias, pre = leaky(z), out = pre + residual -- with what the mutations and the bound need."""

    def __init__(self, case, i, x, mode, res):
        l = case.layers[i]
        self.case, self.i, self.mode, self.x, self.res = case, i, mode, x, res
        self.size, self.stride, self.leaky, self.F = int(l["size"]), int(l["stride"]), bool(l["leaky"]), int(l["filters"])
        assert x.shape[-1] == case.cin(i), "convolution %d reads %d channels, given %d" % (i, case.cin(i), x.shape[-1])
        assert (res is None) == (case.fused(i) is None), "convolution %d: the fused residual must be given exactly when a [shortcut] follows" % i
        self.w, self.b = case.stored(i, mode)
        self.slope = 0.1 if mode == "f64" else float(np.float32(0.1))
        self.z = _conv_nhwc(x, self.w, self.stride) + self.b
        self.out = self.post(self.z)

    def act(self, z):
        return np.where(z > 0, z, self.slope * z) if self.leaky else z

    def post(self, z, res="own"):
        r = self.res if isinstance(res, str) else res
        return self.act(z) + (0 if r is None else r)

    def absolute(self):
        """A = conv(|x|, |w|) + |bias| + |residual|"""
        a = _conv_nhwc(np.abs(self.x), np.abs(self.w), self.stride) + np.abs(self.b)
        return a if self.res is None else a + np.abs(self.res)

    def absolute_winograd(self):
        """A_w: the Winograd expression on absolute values (3 x 3, stride 1), cropped to the map."""
        n, H, W, C = self.x.shape
        th, tw = (H + 1) // 2, (W + 1) // 2
        xp = np.zeros((n, 2 * th + 2, 2 * tw + 2, C))
        xp[:, 1:H + 1, 1:W + 1] = np.abs(self.x)
        # |B^T| |d| |B| per block: the 4 x 4 patches of every 2 x 2 output block
        d = np.stack([np.stack([xp[:, a:a + 2 * th:2, b:b + 2 * tw:2] for b in range(4)], 0) for a in range(4)], 0)      # (4, 4, n, th, tw, C)
        V = np.einsum("ia,abntwc,jb->ijntwc", np.abs(_BT), d, np.abs(_BT))
        Ua = np.einsum("ia,fcab,jb->ijfc", np.abs(_G), np.abs(self.w), np.abs(_G))                                   # (4, 4, F, C)
        M = np.stack([np.stack([V[a, b] @ Ua[a, b].T for b in range(4)], 0) for a in range(4)], 0)                    # (4, 4, n, th, tw, F)
        Y = np.einsum("ia,abntwf,jb->ntiwjf", np.abs(_AT), M, np.abs(_AT)).reshape(n, 2 * th, 2 * tw, self.F)[:, :H, :W]
        Y = Y + np.abs(self.b)
        return Y if self.res is None else Y + np.abs(self.res)

    def bound(self):
        K = self.case.taps_k(self.i)
        if self.case.is_wino(self.i, self.mode):
            return 2 * (self.case.cin(self.i) + 18) * U32 * self.absolute_winograd()
        e = 2 * K * U32 * self.absolute()
        if self.mode in ("f32", "f32w"):
            return e
        if self.mode == "f32x3":
            return e + 2.0 ** -23 * (1 + 2.0 ** -9) * self.absolute() if self.F >= 64 and self.i > 0 else e
        assert self.mode == "f16"
        sub = 2.0 ** -24
        b = e * (1 + 2.0 ** -10) + np.maximum(2.0 ** -11 * np.abs(self.out), sub) + 2.0 ** -23 * np.abs(self.b)
        if self.res is not None:
            b = b + np.maximum(2.0 ** -11 * np.abs(self.act(self.z)), sub)
        return b


# ------------------------------------------------------------------------------------------------------------------------------------
# Mutations: subtly wrong references, each a function of the correct evaluation.  A mutation returns the mutated output, or None where it does
# not apply to the layer.  tests/test_yolo_cases.py asserts that the correct reference plus the bound REJECTS every one of them on every layer
# it applies to -- otherwise the GPU comparison would be vacuous there.
# ------------------------------------------------------------------------------------------------------------------------------------
def _tap(ev, n, yi, xi, kh, kw):
    """contribution of input pixels (n, yi, xi[]) through tap (kh, kw): (len(xi), F)"""
    return ev.x[n, yi, xi, :] @ ev.w[:, :, kh, kw].T


def mut_drop_border_tap(ev):
    """the bottom row of image 0 loses tap (0, 0) -- a tap mask that is wrong at one edge"""
    n, Ho, Wo, _ = ev.z.shape
    if ev.size != 3 or Ho < 2 or Wo < 2:
        return None
    xo = np.arange(1, Wo)
    z = ev.z.copy()
    z[0, Ho - 1, xo] -= _tap(ev, 0, (Ho - 1) * ev.stride - 1, xo * ev.stride - 1, 0, 0)
    return ev.post(z)


def mut_neighbour_image_tap(ev):
    """the top row of image 1 reads its padding row from the bottom row of image 0 -- a flattened pixel index without the image test"""
    n, Ho, Wo, _ = ev.z.shape
    H, W = ev.x.shape[1:3]
    if ev.size != 3 or n < 2:
        return None
    z = ev.z.copy()
    for kw in range(3):
        xo = np.array([v for v in range(Wo) if 0 <= v * ev.stride - 1 + kw < W], dtype=int)
        z[1, 0, xo] += _tap(ev, 0, H - 1, xo * ev.stride - 1 + kw, 0, kw)
    return ev.post(z)


def mut_shift_channel_group(ev):
    """every output lands one channel group of 4 further on"""
    if ev.F < 8:
        return None
    o = np.zeros_like(ev.out)
    o[..., 4:] = ev.out[..., :-4]
    return o


def mut_partial_tile_unwritten(ev):
    """the last filters % 64 channels -- the part of the filters that does not fill a tile -- stay unwritten (zero)"""
    if ev.F % 64 == 0:
        return None
    o = ev.out.copy()
    o[..., ev.F - ev.F % 64:] = 0
    return o


def mut_skip_leaky_one_channel(ev):
    """one channel misses its leaky ReLU (the channel with the most negative pre-activation)"""
    c = int(np.argmin(ev.z.min(axis=(0, 1, 2))))
    if not ev.leaky or ev.z[..., c].min() >= 0:
        return None
    o = ev.out.copy()
    o[..., c] = ev.z[..., c] + (0 if ev.res is None else ev.res[..., c])
    return o


def mut_skip_residual_last_tile(ev):
    """the last pixel tile (128 pixels of the flattened batch) misses its residual"""
    if ev.res is None:
        return None
    o = ev.out.copy().reshape(-1, ev.F)
    o[-128:] -= ev.res.reshape(-1, ev.F)[-128:]
    return o.reshape(ev.out.shape)


def mut_swap_two_filters(ev):
    """filters 0 and 1 change places"""
    if ev.F < 2:
        return None
    o = ev.out.copy()
    o[..., [0, 1]] = o[..., [1, 0]]
    return o


def mut_unpadded_stride_255(ev):
    """a 255-channel tensor written with a pixel stride of 255 and read with its stored stride of 256"""
    npix = ev.out.size // ev.F
    if ev.F != 255 or npix < 2:
        return None
    buf = np.zeros(npix * 256)
    buf[:npix * 255] = ev.out.reshape(-1)
    return buf.reshape(npix, 256)[:, :255].reshape(ev.out.shape)


MUTATIONS = [mut_drop_border_tap, mut_neighbour_image_tap, mut_shift_channel_group, mut_partial_tile_unwritten, mut_skip_leaky_one_channel,
             mut_skip_residual_last_tile, mut_swap_two_filters, mut_unpadded_stride_255]

CASES = [Case("partial", _PARTIAL, 96, 64, (3,), 11, 2.0, -3.0), Case("odd", _ODD, 160, 96, (5,), 12, 4.0, -1.0), Case("wide", _WIDE, 128, 32, (1,), 13, 2.0, -2.5),
         Case("b3f5", _B3F5, 352, 32, (1,), 14, 6.0, -4.0), Case("tiny", _TINY, 32, 32, (1, 96), 15, 12.0, -1.0), Case("dense-route", _DENSE_ROUTE, 64, 64, (2,), 16, 6.0, -6.0),
         Case("no-head", _NO_HEAD, 32, 32, (2,), 17)]
CASE = {c.name: c for c in CASES}
RUNS = [(c.name, b) for c in CASES for b in c.batches]          # every (list, batch) the GPU tests run

# Lists sd_yolo_create_prec must refuse (the forward must never be asked to run them): name -> (layers, net_w, net_h)
REFUSED = {
    "unfused shortcut": ([conv(32), conv(64, 3, 2), conv(64), shortcut(-2), route(-2), conv(64, 1)], 64, 64),     # the convolution's output has a second consumer
    "shortcut onto its own convolution": ([conv(32), conv(32), shortcut(-1)], 64, 64),
    "stand-alone upsample": ([conv(32), conv(64, 3, 2), upsample(), conv(32, 1)], 64, 64),
    "upsample read by a 1-input route": ([conv(32), conv(64, 3, 2), upsample(), route(-1, 0), route(-2)], 64, 64),
    "2-input route without an upsample": ([conv(32), conv(32), route(-1, -2), conv(64, 1)], 64, 64),
    "input channels 48": ([conv(32), conv(48), conv(64)], 64, 64),
    "5 x 5 convolution": ([conv(32), conv(64, 5)], 64, 64),
    "stride 3": ([conv(32), conv(64, 3, 3)], 64, 64),
    "first layer with 64 filters": ([conv(64), conv(64)], 64, 64),
    "first layer 1 x 1": ([conv(32, 1), conv(64)], 64, 64),
    "head of 254 channels": ([conv(32), conv(254, 1, 1, 0, 0), yolo(0, 1, 2)], 64, 64),
    "route copy of a 255-channel tensor": ([conv(32), conv(64, 3, 2), head(), upsample(), route(-1, 0)], 64, 64),
}


# ------------------------------------------------------------------------------------------------------------------------------------
# The planner (csrc/sd_yolo_plan.h through tests/cpp/yolo_plan_dump.cpp, g++ alone)
# ------------------------------------------------------------------------------------------------------------------------------------
_DUMP = []


def plan_dump_exe():
    if not _DUMP:
        d = tempfile.mkdtemp(prefix="yolo_cases_plan_")
        exe = os.path.join(d, "yolo_plan_dump")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "slam-dynamic_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "yolo_plan_dump.cpp")])
        _DUMP.append((d, exe))
    return _DUMP[0]


def plan_many(items):
    """items: [(layers, net_w, net_h, mode, batch)] -> per item {"convs": {layer: (kernel, {launch fields}, filters, size, cinPad, class)},
    "routes": {layer: "inplace" | "copy"}} or {"refused": (code, text)}; one process for all of them."""
    d, exe = plan_dump_exe()
    args = []
    for k, (layers, w, h, mode, batch) in enumerate(items):
        path = os.path.join(d, "list_%d.txt" % k)
        with open(path, "w") as f:
            for l in layer_array(layers) if not isinstance(layers, np.ndarray) else layers:
                f.write(" ".join(str(int(v)) for v in (l["type"], l["filters"], l["size"], l["stride"], l["batch_normalize"], l["leaky"], l["from"][0], l["from"][1],
                                                       l["nfrom"], l["mask"][0], l["mask"][1], l["mask"][2])) + "\n")
        args += ["--layers", path, str(PRECS[mode]), str(w), str(h), str(batch)]
    out, cur = [], None
    for line in subprocess.check_output([exe] + args, text=True).splitlines():
        if line.startswith("case "):
            cur = {"convs": {}, "routes": {}}
            out.append(cur)
        elif line.startswith("refused|"):
            _, code, text = line.split("|", 2)
            cur.clear()
            cur["refused"] = (int(code), text)
        elif line.startswith("route|"):
            _, layer, how = line.split("|")
            cur["routes"][int(layer)] = how
        else:
            layer, kernel, nums, shape = line.split("|")
            gx, gy, block, tx, ty, g, width, pre = (int(v) for v in nums.split())
            filters, size, cin, cls = (int(v) for v in shape.split())
            cur["convs"][int(layer)] = (kernel, dict(gridX=gx, gridY=gy, block=block, tilesX=tx, tilesY=ty, groupY=g, width=width, inputGrid=pre), filters, size, cin, cls)
    assert len(out) == len(items)
    return out


def plan(case, mode, batch):
    return plan_many([(case.layers, case.net_w, case.net_h, mode, batch)])[0]
